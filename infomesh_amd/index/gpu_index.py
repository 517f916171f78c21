"""GPU hybrid index shard: segmented CSR inverted index (BM25) + dense
embeddings (cosine) resident in HBM3E, scored by hand-written CDNA4
kernels.

Replaces intra-node: SQLite FTS5 MATCH+bm25() (reference
infomesh/index/local_store.py:316-332) and ChromaDB HNSW
(infomesh/index/vector_store.py:92-254). One shard per GPU; documents
hash-partitioned across shards; the query plane (parallel/query_plane.py)
fans out and all-gathers top-k.

Segmented design (the FTS5 append/optimize analogue, reference
local_store.py:528-541): a flush appends ONE new posting segment built
only from the new docs — O(new), no host pull-back of old postings —
and `optimize()` merges segments GPU-side (torch sort over (term, doc)
keys). BM25 stays exact across segments because the per-posting doc
length travels packed with tf and the norm is computed in-kernel from
the CURRENT global avgdl; idf comes from the global df table summed
over segments. Segments partition the doc-id axis, so per-segment
score kernels write disjoint column ranges of the [B, N] score matrix
(each column exactly once — no zero-fill, no atomics across segments).

Shard sizing: 1.25M docs × (≈120 postings × 8 B + 384 × 2 B embedding)
≈ 2.2 GB — far under the 288 GB HBM budget, so shards scale to 100M+
docs per GPU; the bench uses the BASELINE 10M-doc/8-GPU config.
"""
from __future__ import annotations

import math
import os
import re
from dataclasses import dataclass

import numpy as np
import torch

from ..hashing import hash64
from .doc_attrs import (DEAD_BIT, TOP_FETCH, U32_MAX, DocFilter, FacetSpec,
                        TermOps, domain_tables_np, domain_top_np,
                        facet_counts_np, pack_facets, pack_pred,
                        pack_pred_sets, passes, words_i32)

BM25_K1 = 1.2
BM25_B = 0.75
BM25_VOCAB = 1 << 17

# auto-merge threshold: beyond this many live segments a flush triggers
# optimize() (GPU-side merge) — the FTS5 automerge analogue
MAX_SEGMENTS = 16

# per-domain cap (ops/csrc/collapse.hip): the largest m a row may ask
# for, and the most the [m, R, D] u64 workspace of one plane may take;
# more capped rows than fit are processed in slices
COLLAPSE_M_MAX = 4
COLLAPSE_WS_BYTES = 256 << 20


def per_domain_caps(per_domain, B: int) -> list[int] | None:
    """One cap per row from a per_domain argument (one int or None per
    row, or None): None when no row is capped. A cap outside
    0 .. COLLAPSE_M_MAX is a ValueError."""
    if per_domain is None:
        return None
    caps = [int(m or 0) for m in per_domain]
    assert len(caps) == B, "per_domain: one entry per query"
    if any(not 0 <= m <= COLLAPSE_M_MAX for m in caps):
        raise ValueError(
            f"per_domain: {caps}; 0 (no cap) or 1 <= m <= {COLLAPSE_M_MAX}")
    return caps if any(caps) else None


def _mask_kw(mask) -> dict:
    """A plane's mask, (bits, row_pred) or None, as the mask= / row_pred=
    keywords of the ops.kernels calls."""
    bits, row_pred = mask if mask is not None else (None, None)
    return {"mask": bits, "row_pred": row_pred}


# \w+ covers all unicode letters/digits (FTS5 unicode61 analogue);
# diacritics are NFKD-folded below like unicode61 remove_diacritics
_WORD_RE = re.compile(r"\w+")


def bm25_term_ids(text: str, vocab: int = BM25_VOCAB) -> np.ndarray:
    """Tokenize + hash into the BM25 term space. A registered
    'tokenizer' plugin (utils/plugins.py, reference dx.py:153-188)
    replaces the default word tokenizer for BOTH indexing and queries
    — the hash space keeps them consistent automatically.

    CJK runs are expanded into character bigrams (the GPU analogue of
    the reference's FTS5 trigram/CJK handling, search/cjk.py): the
    default latin word regex alone would drop CJK text entirely from
    the GPU BM25 plane."""
    from ..utils.plugins import GLOBAL_PLUGINS
    tok = GLOBAL_PLUGINS.get_single("tokenizer")
    if tok is not None:
        toks = tok(text)
    else:
        if any(ord(c) > 127 for c in text):
            # diacritic folding (cafe == café), matching the FTS5
            # unicode61 tokenizer's remove_diacritics so both score
            # planes see the same terms
            import unicodedata
            text = "".join(c for c in unicodedata.normalize("NFKD", text)
                           if not unicodedata.combining(c))
        toks = _WORD_RE.findall(text.lower())
        # fast ordinal check before paying the regex: any char >= U+2E80
        if any(ord(c) >= 0x2E80 for c in text):
            from ..search.cjk import _CJK_RUN_RE, ngram_expand
            for m in _CJK_RUN_RE.finditer(text):
                toks.extend(ngram_expand(m.group(0), 2))
    if not toks:
        return np.zeros(0, dtype=np.int64)
    return np.fromiter((hash64(t) % vocab for t in toks), dtype=np.int64,
                       count=len(toks))


@dataclass
class DomainTally:
    """A shard's per-domain match counts of one batch's top rows, kept
    for the query plane's second round: cnt [Rt, D] i32 over the shard's
    domain ids, dom_keys [D] i32, the ids' hashes (u32 bits, ascending
    as unsigned). cnt may be the shard's workspace: it holds until the
    shard's next batch."""
    cnt: torch.Tensor
    dom_keys: torch.Tensor

    def lookup(self, hashes: torch.Tensor) -> torch.Tensor:
        """hashes [Rt, U] (u32 bits, any integer dtype) -> [Rt, U] i32:
        row r's count of every hash, 0 for one the shard does not hold."""
        keys = self.dom_keys.long() & U32_MAX
        h = hashes.to(keys.device).long() & U32_MAX
        pos = torch.searchsorted(keys, h).clamp(max=keys.numel() - 1)
        got = self.cnt.gather(1, pos)
        return torch.where(keys[pos] == h, got, torch.zeros_like(got))


@dataclass
class ShardHits:
    """Fixed-size per-shard top-k results (scores + GLOBAL doc ids)."""
    bm25_scores: torch.Tensor   # [B, k] f32
    bm25_ids: torch.Tensor      # [B, k] i64 (-1 pad)
    dense_scores: torch.Tensor  # [B, k] f32
    dense_ids: torch.Tensor     # [B, k] i64
    # [R, F] i32 facet counts of the rows a FacetSpec names (layout:
    # ops/csrc/facets.hip); None when the caller asked for none
    facets: torch.Tensor | None = None
    # [Rt, TOP_FETCH + 1, 2] i32 (hash bits, count) pairs: the shard's
    # first domains of every row that asked for top domains, in order
    # (ops/csrc/domtop.hip), and the tally they were selected from; None
    # when no row asked
    dom_top: torch.Tensor | None = None
    dom_tally: DomainTally | None = None
    # [B, k] i32: the hits' domain words (w2 of the attribute record, 0
    # at padding), for the query plane's cap on the merged lists; None
    # when no row of the batch carries a per-domain cap
    bm25_dom: torch.Tensor | None = None
    dense_dom: torch.Tensor | None = None


@dataclass
class PostingSegment:
    """One immutable CSR posting segment covering the doc-id range
    [doc_base, doc_base + n_docs)."""
    offsets: torch.Tensor   # [V+1] i64 (device)
    doc_ids: torch.Tensor   # [P] i32, SEGMENT-local ids, asc per term
    tfdl: torch.Tensor      # [P] i32: tf | (dl << 16)
    doc_base: int
    n_docs: int
    h_offs: np.ndarray      # host copy of offsets (query-time chunking)

    def hbm_bytes(self) -> int:
        return sum(t.numel() * t.element_size()
                   for t in (self.offsets, self.doc_ids, self.tfdl))


class GpuShard:
    """One GPU's slice of the hybrid index."""

    def __init__(self, device: str = "cuda", vocab: int = BM25_VOCAB,
                 emb_dtype: str = "bf16"):
        assert emb_dtype in ("bf16", "fp8")
        self.device = torch.device(device)
        self.vocab = vocab
        # "fp8" stores embeddings as OCP e4m3 (half the HBM + half the
        # dense-plane read traffic; ~0.4% relative score error on
        # unit-norm vectors) — opt-in via config gpu.dtype
        self.emb_dtype = emb_dtype
        self.n_docs = 0
        self.segments: list[PostingSegment] = []
        self.df: np.ndarray = np.zeros(vocab, dtype=np.int64)  # global df
        self._doc_lens = np.zeros(0, dtype=np.int64)           # host [N]
        self.avgdl = 1.0
        # dense plane: capacity-growth device buffers ([:n_docs] live)
        self._emb_buf: torch.Tensor | None = None   # [cap, D] bf16 (unit)
        self._gid_buf: torch.Tensor | None = None   # [cap] i64
        # filter attributes, one 16-byte record per doc (doc_attrs.py);
        # bit 16 of word 1 is the tombstone set by delete()
        self._attr_buf: torch.Tensor | None = None  # [cap, 4] i32
        self.n_dead = 0
        self._live_bits = None   # cached live-only mask (+ ready event)
        # per-epoch domain tables (dom_keys [D], dom_id [N]), built by
        # the first request for top domains, and the [R, D] count
        # workspace of ops/csrc/domtop.hip
        self._dom_tables = None
        self._dom_ws: torch.Tensor | None = None
        # [m, R, D] u64 workspaces of ops/csrc/collapse.hip, one per
        # plane (the planes may run on two streams)
        self._collapse_ws: dict[str, torch.Tensor] = {}
        self._topk = None
        self._topk_dense = None
        # selectors over block maxima, one per plane (the planes may run
        # on two streams, and a wide shard gives each a workspace)
        self._topk_pruned = None
        self._topk_pruned_bm25 = None
        self._dense_bmax: dict = {}  # [B, NB] block maxima, per B
        # BM25 plane from block maxima (bm25_block(bmax=) + TopKPruned,
        # W = 64) on unmasked batches of a shard whose segments all start
        # at a multiple of 64; off (also INFOMESH_BM25_PRUNED=0, for
        # measuring the two apart) = always the fused histogram + TopK
        self.bm25_pruned = os.environ.get("INFOMESH_BM25_PRUNED") != "0"
        self._bm25_bmax: dict = {}   # [B, ceil(N/64)] block maxima, per B
        self._dense_graphs: dict = {}
        # hipGraph-capture the dense plane; set by the overlapped query
        # plane, off for direct search() callers
        self.graph_dense = False
        self._h_idf: np.ndarray | None = None
        # pending (un-built) batch buffers — the ingest side-buffer;
        # GPU visibility flips at build() (epoch-style).
        self._pend_tokens: list[np.ndarray] = []
        self._pend_emb: list[torch.Tensor] = []
        self._pend_gids: list[int] = []
        self._pend_attrs: list = []

    # ------------------------------------------------- derived views
    @property
    def embeddings(self) -> torch.Tensor | None:
        if self._emb_buf is None or self.n_docs == 0:
            return None
        return self._emb_buf[:self.n_docs]

    @property
    def global_ids(self) -> torch.Tensor | None:
        if self._gid_buf is None:
            return None
        return self._gid_buf[:self.n_docs]

    @property
    def attrs(self) -> torch.Tensor | None:
        if self._attr_buf is None:
            return None
        return self._attr_buf[:self.n_docs]

    @property
    def doc_norm(self) -> torch.Tensor:
        """BM25 length norm per doc (host-derived; kernels compute this
        in-flight from packed dl — kept for the CPU oracle/tests)."""
        dl = self._doc_lens.astype(np.float32)
        return torch.from_numpy(
            BM25_K1 * (1 - BM25_B + BM25_B * dl / self.avgdl))

    # ------------------------------------------------------------ build
    def add_document(self, global_id: int, term_ids: np.ndarray,
                     embedding: torch.Tensor | None,
                     attrs=None) -> None:
        """attrs: the 4 words of doc_attrs.pack_attrs, or None for an
        all-zero record (no language, no date, no domain)."""
        self._pend_tokens.append(term_ids.astype(np.int64))
        self._pend_gids.append(global_id)
        self._pend_attrs.append(attrs)
        if embedding is not None:
            self._pend_emb.append(embedding.reshape(1, -1))

    def build(self) -> None:
        """Make pending docs searchable by appending ONE new posting
        segment — O(new docs), never O(corpus). Triggers a GPU-side
        optimize() merge when the segment count exceeds MAX_SEGMENTS
        (the FTS5 automerge analogue)."""
        if not self._pend_tokens:
            return
        token_lists = self._pend_tokens
        gids = list(self._pend_gids)
        embs = self._pend_emb
        attrs = self._pend_attrs
        self._pend_tokens, self._pend_gids, self._pend_emb = [], [], []
        self._pend_attrs = []
        new_emb = torch.cat(embs, 0) if embs else None
        self._append_segment(token_lists, gids, new_emb, attrs=attrs)
        if len(self.segments) > MAX_SEGMENTS:
            self.optimize()

    def merged_with(self, token_lists: list[np.ndarray],
                    gids: list[int],
                    new_emb: torch.Tensor | None,
                    attrs=None) -> "GpuShard":
        """Return a NEW shard = this shard + the given docs, sharing
        the immutable segments/buffers with this one (epoch-flip:
        readers of the old shard never see the new docs because every
        read is bounded by the old n_docs). Linear use only — append to
        the RETURNED shard, not to this one, afterwards. The attribute
        buffer is shared too, so a delete() on either shard tombstones
        the common rows for both at once."""
        out = type(self)() if type(self).__init__ is not GpuShard.__init__ \
            else GpuShard(str(self.device), vocab=self.vocab,
                          emb_dtype=self.emb_dtype)
        out.vocab = self.vocab
        out.emb_dtype = self.emb_dtype
        out.n_docs = self.n_docs
        out.segments = list(self.segments)
        out.df = self.df.copy()
        out._doc_lens = self._doc_lens
        out.avgdl = self.avgdl
        out._emb_buf = self._emb_buf
        out._gid_buf = self._gid_buf
        out._attr_buf = self._attr_buf
        out.n_dead = self.n_dead
        out._append_segment(token_lists, gids, new_emb, attrs=attrs)
        return out

    def _append_segment(self, token_lists: list[np.ndarray],
                        gids: list, new_emb: torch.Tensor | None,
                        attrs=None) -> None:
        lens2 = np.array([max(len(t), 1) for t in token_lists],
                         dtype=np.int64)
        flat_terms = (np.concatenate(
            [t.astype(np.int64) for t in token_lists])
            if any(len(t) for t in token_lists)
            else np.zeros(0, np.int64))
        flat_docs = np.repeat(np.arange(len(token_lists), dtype=np.int64),
                              [len(t) for t in token_lists])
        self._install_segment(flat_terms, flat_docs, lens2,
                              np.asarray(gids, dtype=np.int64), new_emb,
                              attrs)

    def build_from_arrays(self, flat_terms: np.ndarray,
                          flat_docs: np.ndarray, doc_lens: np.ndarray,
                          global_ids: np.ndarray,
                          embeddings: torch.Tensor | None,
                          attrs=None) -> None:
        """Bulk build from flat (term, doc-local-id) pairs — installs a
        single segment (doc ids must be 0..len(doc_lens)-1)."""
        self._install_segment(flat_terms, flat_docs,
                              np.asarray(doc_lens, dtype=np.int64),
                              np.asarray(global_ids, dtype=np.int64),
                              embeddings, attrs)

    @staticmethod
    def _attr_rows(attrs, n: int) -> np.ndarray | None:
        """attrs argument -> [n, 4] int32 words, or None when every
        record is all-zero. Accepts an [n, 4] array or a list whose
        entries are 4 words or None."""
        if attrs is None:
            return None
        if isinstance(attrs, np.ndarray):
            rows = attrs.reshape(-1, 4)
            rows = (rows.view(np.int32) if rows.dtype.itemsize == 4
                    else words_i32(rows))
        else:
            if all(a is None for a in attrs):
                return None
            rows = words_i32([a if a is not None else (0, 0, 0, 0)
                              for a in attrs])
        assert rows.shape == (n, 4), "one attribute record per document"
        return rows

    @staticmethod
    def _aggregate(flat_terms: np.ndarray, flat_docs: np.ndarray,
                   n: int) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(term, doc) pairs -> unique pairs + tf counts, term-sorted."""
        key = flat_terms * np.int64(max(n, 1)) + flat_docs
        key.sort(kind="stable")
        uniq, counts = np.unique(key, return_counts=True)
        terms_u = (uniq // max(n, 1)).astype(np.int64)
        docs_u = (uniq % max(n, 1)).astype(np.int32)
        tf_u = np.minimum(counts, 65535).astype(np.uint16)
        return terms_u, docs_u, tf_u

    def _upload(self, arr: np.ndarray, stream) -> torch.Tensor:
        """Host -> HBM via a pinned staging buffer on the ingest side
        stream (hipMemcpyAsync under the hood) so uploads overlap any
        query work on the compute stream — SURVEY.md §5.8 ingest path."""
        t = torch.from_numpy(np.ascontiguousarray(arr))
        if stream is None:
            return t.clone()
        pinned = t.pin_memory()
        with torch.cuda.stream(stream):
            return pinned.to(self.device, non_blocking=True)

    def _grow(self, buf: torch.Tensor | None, need: int,
              row_shape: tuple, dtype: torch.dtype) -> torch.Tensor:
        """Capacity-doubling device buffer growth (amortized O(1) per
        append; the old tensor stays valid for prior-epoch readers)."""
        if buf is None:
            cap = max(need, 256)
            return torch.empty((cap, *row_shape), device=self.device,
                               dtype=dtype)
        if buf.shape[0] >= need:
            return buf
        cap = max(need, 2 * buf.shape[0])
        new = torch.empty((cap, *row_shape), device=self.device,
                          dtype=dtype)
        new[:self.n_docs] = buf[:self.n_docs]
        return new

    def _install_segment(self, flat_terms: np.ndarray,
                         flat_docs: np.ndarray, doc_lens: np.ndarray,
                         global_ids: np.ndarray,
                         embeddings: torch.Tensor | None,
                         attrs=None) -> None:
        n_new = len(doc_lens)
        if n_new == 0:
            return
        if self.n_docs > 0:
            assert (embeddings is not None) == (self._emb_buf is not None), \
                "dense/sparse mode must be consistent across appends"
        on_gpu = self.device.type == "cuda"
        stream = torch.cuda.Stream(self.device) if on_gpu else None
        if stream is not None:
            # new_emb may have been produced on the compute stream
            # (encoder output): order the side-stream copies after it
            stream.wait_stream(torch.cuda.current_stream(self.device))
        if on_gpu and len(flat_terms) > 2_000_000:
            # bulk builds aggregate ON-DEVICE: the host (term,doc) key
            # sort took ~120 s for the 10M-doc corpus (567M postings);
            # torch's GPU radix sort + unique_consecutive do it in
            # seconds. Small appends keep the host path (cheaper than
            # the round trip).
            seg, df_new = self._aggregate_device(
                flat_terms, flat_docs, doc_lens, n_new)
        else:
            terms_u, docs_u, tf_u = self._aggregate(flat_terms,
                                                    flat_docs, n_new)
            dl_u = np.minimum(doc_lens[docs_u.astype(np.int64)], 65535)
            tfdl = (tf_u.astype(np.uint32)
                    | (dl_u.astype(np.uint32) << np.uint32(16))
                    ).view(np.int32)
            df_new = np.bincount(terms_u,
                                 minlength=self.vocab).astype(np.int64)
            offsets = np.zeros(self.vocab + 1, dtype=np.int64)
            np.cumsum(df_new, out=offsets[1:])
            seg = PostingSegment(
                offsets=self._upload(offsets, stream),
                doc_ids=self._upload(docs_u.astype(np.int32), stream),
                tfdl=self._upload(tfdl, stream),
                doc_base=self.n_docs, n_docs=n_new, h_offs=offsets)
        # dense-plane buffers: append rows [n_docs : n_docs+n_new]
        need = self.n_docs + n_new
        self._gid_buf = self._grow(self._gid_buf, need, (), torch.int64)
        gid_t = self._upload(global_ids.astype(np.int64), stream)
        self._attr_buf = self._grow(self._attr_buf, need, (4,), torch.int32)
        attr_rows = self._attr_rows(attrs, n_new)
        attr_t = (self._upload(attr_rows, stream)
                  if attr_rows is not None else None)

        def put_attrs():
            if attr_t is None:
                self._attr_buf[self.n_docs:need].zero_()
            else:
                self._attr_buf[self.n_docs:need].copy_(attr_t)
        if stream is not None:
            with torch.cuda.stream(stream):
                put_attrs()
        else:
            put_attrs()
        if embeddings is not None:
            e = embeddings
            store_dtype = (torch.float8_e4m3fn if self.emb_dtype == "fp8"
                           else torch.bfloat16)
            if e.dtype not in (torch.bfloat16, torch.float8_e4m3fn):
                e = torch.nn.functional.normalize(e.float(), dim=-1)
            if e.dtype != store_dtype:
                e = e.to(store_dtype)
            assert e.shape[0] == n_new, \
                "dense shard requires embeddings for every pending doc"
            self._emb_buf = self._grow(self._emb_buf, need,
                                       (e.shape[1],), store_dtype)
            if e.device.type == "cpu" and self.device.type == "cuda":
                e = self._upload_t(e, stream)
            if stream is not None:
                with torch.cuda.stream(stream):
                    self._emb_buf[self.n_docs:need].copy_(e)
                    self._gid_buf[self.n_docs:need].copy_(gid_t)
            else:
                self._emb_buf[self.n_docs:need].copy_(e)
                self._gid_buf[self.n_docs:need].copy_(gid_t)
        else:
            if stream is not None:
                with torch.cuda.stream(stream):
                    self._gid_buf[self.n_docs:need].copy_(gid_t)
            else:
                self._gid_buf[self.n_docs:need].copy_(gid_t)
        if stream is not None:
            # epoch flip: the segment becomes visible only after the
            # side stream's uploads complete on the compute stream.
            torch.cuda.current_stream(self.device).wait_stream(stream)
        self.segments.append(seg)
        self.df = self.df + df_new
        self._doc_lens = np.concatenate([self._doc_lens, doc_lens])
        self.avgdl = float(self._doc_lens.mean())
        self.n_docs = need
        self._invalidate_query_caches()

    def _aggregate_device(self, flat_terms: np.ndarray,
                          flat_docs: np.ndarray, doc_lens: np.ndarray,
                          n_new: int):
        """GPU bulk aggregation: (term, doc) pairs -> term-sorted CSR
        postings with packed tf|dl, entirely on-device."""
        dev = self.device
        t = torch.from_numpy(np.ascontiguousarray(flat_terms)).to(dev)
        d = torch.from_numpy(np.ascontiguousarray(flat_docs)).to(dev)
        key, _ = torch.sort(t * np.int64(max(n_new, 1)) + d)
        del t, d
        uniq, counts = torch.unique_consecutive(key, return_counts=True)
        del key
        terms_u = uniq // max(n_new, 1)
        docs_u = (uniq % max(n_new, 1)).to(torch.int32)
        del uniq
        tf = counts.clamp(max=65535).to(torch.int32)
        dl_dev = torch.from_numpy(
            np.minimum(doc_lens, 65535).astype(np.int64)).to(dev)
        dl = dl_dev[docs_u.long()].to(torch.int32)
        tfdl = (tf | (dl << 16)).contiguous()
        df_dev = torch.bincount(terms_u, minlength=self.vocab)
        offsets_dev = torch.zeros(self.vocab + 1, dtype=torch.int64,
                                  device=dev)
        torch.cumsum(df_dev, 0, out=offsets_dev[1:])
        df_new = df_dev.cpu().numpy().astype(np.int64)
        seg = PostingSegment(
            offsets=offsets_dev, doc_ids=docs_u.contiguous(),
            tfdl=tfdl, doc_base=self.n_docs, n_docs=n_new,
            h_offs=offsets_dev.cpu().numpy())
        return seg, df_new

    def _upload_t(self, t: torch.Tensor, stream) -> torch.Tensor:
        pinned = t.contiguous().pin_memory()
        with torch.cuda.stream(stream):
            return pinned.to(self.device, non_blocking=True)

    def _invalidate_query_caches(self) -> None:
        self._h_idf = None
        # dense hipGraphs captured the old embeddings view/shape
        self._dense_graphs = {}
        self._dense_bufs = {}
        self._dense_bmax = {}
        self._bm25_bmax = {}
        self._bm25_hists = {}
        self._live_bits = None
        # n_docs or the row order changed (a delete alone sets a dead
        # bit and keeps them)
        self._dom_tables = None
        self._dom_ws = None

    def optimize(self) -> None:
        """Merge all posting segments into one, entirely on-device:
        reconstruct (term, global-doc) keys, single torch.sort, gather
        tfdl — the FTS5 `optimize()` analogue (reference
        local_store.py:528-541). Docs never repeat across segments, so
        no tf re-aggregation is needed."""
        if len(self.segments) <= 1:
            return
        dev = self.device
        V = self.vocab
        term_parts, doc_parts, tfdl_parts = [], [], []
        arangeV = torch.arange(V, dtype=torch.int64, device=dev)
        for seg in self.segments:
            dfg = seg.offsets.diff()
            term_parts.append(torch.repeat_interleave(arangeV, dfg))
            doc_parts.append(seg.doc_ids.to(torch.int64) + seg.doc_base)
            tfdl_parts.append(seg.tfdl)
        terms = torch.cat(term_parts)
        docs = torch.cat(doc_parts)
        tfdl = torch.cat(tfdl_parts)
        key = terms * self.n_docs + docs
        key, order = torch.sort(key)
        docs_sorted = (key % self.n_docs).to(torch.int32)
        tfdl_sorted = tfdl[order].contiguous()
        offsets = torch.zeros(V + 1, dtype=torch.int64, device=dev)
        torch.cumsum(torch.from_numpy(self.df).to(dev), 0,
                     out=offsets[1:])
        self.segments = [PostingSegment(
            offsets=offsets, doc_ids=docs_sorted, tfdl=tfdl_sorted,
            doc_base=0, n_docs=self.n_docs,
            h_offs=offsets.cpu().numpy())]
        self._invalidate_query_caches()

    # ---------------------------------------------------------- deletes
    def delete(self, global_ids) -> int:
        """Tombstone every row whose global id is in `global_ids`;
        returns how many rows were newly marked dead. One O(N) device
        `isin` — deletes are rare, so no host id map that grows with
        the corpus. The attribute buffer is shared between epochs
        (merged_with), so a delete shows at once, without a flush.

        Tombstoned rows keep counting in `df`, `avgdl` and `n_docs`
        (hence in every idf) until purge() — the Lucene convention:
        scores of live documents do not move when a neighbour dies."""
        ids = np.unique(np.asarray(list(global_ids), dtype=np.int64))
        if self.n_docs == 0 or ids.size == 0:
            return 0
        w1 = self._attr_buf[:self.n_docs, 1]
        hit = torch.isin(self.global_ids, torch.from_numpy(ids).to(self.device))
        hit &= (w1 & DEAD_BIT) == 0
        n = int(hit.sum())
        if n:
            w1 |= hit.to(torch.int32) * DEAD_BIT
            self.n_dead += n
            self._live_bits = None
        return n

    def purge(self) -> int:
        """Physically drop tombstoned rows, on the shard's device (as
        optimize() merges there): rebuild (term, doc, tfdl) from the
        segments keeping live docs, renumber them densely, recompute
        df / doc lengths / avgdl, compact the embedding, id and
        attribute buffers and install ONE segment. Afterwards the shard
        equals one bulk-built from the survivors. Returns the number of
        rows dropped."""
        if self.n_dead == 0:
            return 0
        dev, V, n_old = self.device, self.vocab, self.n_docs
        live = (self._attr_buf[:n_old, 1] & DEAD_BIT) == 0
        new_id = torch.cumsum(live, 0) - 1
        keep_rows = live.nonzero().squeeze(1)
        n_new = int(keep_rows.numel())
        term_parts, doc_parts, tfdl_parts = [], [], []
        arangeV = torch.arange(V, dtype=torch.int64, device=dev)
        for seg in self.segments:
            term_parts.append(
                torch.repeat_interleave(arangeV, seg.offsets.diff()))
            doc_parts.append(seg.doc_ids.to(torch.int64) + seg.doc_base)
            tfdl_parts.append(seg.tfdl)
        terms, docs = torch.cat(term_parts), torch.cat(doc_parts)
        tfdl = torch.cat(tfdl_parts)
        keep = live[docs]
        terms, docs, tfdl = terms[keep], new_id[docs[keep]], tfdl[keep]
        key, order = torch.sort(terms * max(n_new, 1) + docs)
        df_dev = torch.bincount(terms, minlength=V)
        offsets = torch.zeros(V + 1, dtype=torch.int64, device=dev)
        torch.cumsum(df_dev, 0, out=offsets[1:])
        dropped = n_old - n_new
        self.df = df_dev.cpu().numpy().astype(np.int64)
        self._doc_lens = self._doc_lens[live.cpu().numpy()]
        self.avgdl = float(self._doc_lens.mean()) if n_new else 1.0
        self._gid_buf = self._gid_buf.index_select(0, keep_rows)
        self._attr_buf = self._attr_buf.index_select(0, keep_rows)
        if self._emb_buf is not None:
            self._emb_buf = self._emb_buf.index_select(0, keep_rows)
        self.n_docs = n_new
        self.n_dead = 0
        self.segments = [PostingSegment(
            offsets=offsets,
            doc_ids=(key % max(n_new, 1)).to(torch.int32),
            tfdl=tfdl[order].contiguous(), doc_base=0, n_docs=n_new,
            h_offs=offsets.cpu().numpy())] if n_new else []
        self._invalidate_query_caches()
        return dropped

    # ---------------------------------------------------------- filters
    def _pred_rows(self, filters, B: int):
        """None when the mask is inactive (no filter in the batch and
        no tombstone in the shard), else (preds [P, 4] i32 host words,
        row_pred [B] host i32, lists) with the batch's predicates
        deduped; a None filter is the live-only predicate. lists is
        None when no predicate carries a domain list, else one
        (allow_hashes, block_hashes) pair per predicate. A filter is a
        DocFilter, packed words, or the (words, allow, block) form the
        query plane forwards."""
        if self.n_dead == 0 and (filters is None
                                 or all(f is None for f in filters)):
            return None
        if filters is None:
            filters = [None] * B
        assert len(filters) == B, "one filter (or None) per query"
        seen: dict = {}
        rows = [seen.setdefault(pack_pred_sets(f), len(seen))
                for f in filters]
        lists = None
        if any(allow or block for _, allow, block in seen):
            lists = [(allow, block) for _, allow, block in seen]
        return (words_i32([words for words, _, _ in seen]),
                np.asarray(rows, dtype=np.int32), lists)

    @staticmethod
    def _list_tables(lists) -> tuple[np.ndarray, np.ndarray]:
        """Per-predicate (allow, block) hash tuples -> (desc [P, 4] i32,
        doms flat i32 with the u32 bits) as filter_bitmask_sets reads
        them."""
        desc = np.zeros((len(lists), 4), dtype=np.int32)
        flat: list[int] = []
        for p, (allow, block) in enumerate(lists):
            desc[p] = (len(flat), len(allow),
                       len(flat) + len(allow), len(block))
            flat.extend(allow)
            flat.extend(block)
        return desc, np.asarray(flat, dtype=np.uint32).view(np.int32)

    @staticmethod
    def _term_rows(term_ops, B: int) -> list[tuple[int, TermOps]]:
        """(query row, its TermOps) of every row that has an operand."""
        if term_ops is None:
            return []
        assert len(term_ops) == B, "one TermOps (or None) per query"
        return [(i, t) for i, t in enumerate(term_ops) if t]

    def _term_table(self, ops: list[TermOps]):
        """The operand table of csrc/termmask.hip for these rows:
        (op_off [R+1] i32, op_kind [T] i32, ids [T] i64), host arrays;
        a row's require operands come before its exclude operands."""
        op_off = np.zeros(len(ops) + 1, dtype=np.int32)
        np.cumsum([len(t.require) + len(t.exclude) for t in ops],
                  out=op_off[1:])
        ids = np.asarray([i for t in ops for i in t.require + t.exclude],
                         dtype=np.int64)
        kind = np.asarray([k for t in ops for k in
                           [0] * len(t.require) + [1] * len(t.exclude)],
                          dtype=np.int32)
        assert (ids < self.vocab).all(), "term id outside the vocabulary"
        return op_off, kind, ids

    def _mask_for(self, filters: list[DocFilter | None] | None, B: int,
                  term_ops: list[TermOps | None] | None = None):
        """(bits [P, W] i32, row_pred [B] i32) on the device for the
        masked top-k, or None when the mask is inactive. Rows with term
        operands get a bit row of their own, appended after the P
        predicate rows: their predicate's bits with the documents
        cleared that termmask.hip fails."""
        trows = self._term_rows(term_ops, B)
        mask = self._filter_mask_for(filters, B, force=bool(trows))
        if mask is None:
            return None
        bits, h_rows = mask
        if not trows:
            return bits, torch.from_numpy(h_rows).to(self.device)
        from ..ops import kernels as K
        op_off, kind, ids = self._term_table([t for _, t in trows])
        segs = [(seg.doc_ids, seg.doc_base, seg.n_docs,
                 torch.from_numpy(seg.h_offs[ids]),
                 torch.from_numpy(seg.h_offs[ids + 1]))
                for seg in self.segments]
        qrows = np.asarray([i for i, _ in trows], dtype=np.int64)
        # a fresh [R, W] tensor: the (possibly cached) predicate rows
        # are only read
        term_bits = K.term_bitmask(
            bits, torch.from_numpy(h_rows[qrows].astype(np.int64)), segs,
            torch.from_numpy(op_off), torch.from_numpy(kind), self.n_docs)
        h_rows = h_rows.copy()
        h_rows[qrows] = bits.shape[0] + np.arange(len(trows), dtype=np.int32)
        return (torch.cat([bits, term_bits]),
                torch.from_numpy(h_rows).to(self.device))

    def _filter_mask_for(self, filters, B: int, force: bool = False):
        """(bits [P, W] i32 on the device, row_pred [B] i32 on the
        host) of the batch's filters and the shard's tombstones, or
        None when that mask is inactive. force: build it all the same
        (live-only rows), for a batch that needs bit rows to start
        from."""
        from ..ops import kernels as K
        pr = self._pred_rows(filters, B)
        if pr is None and force:
            pr = (words_i32([pack_pred(None)]), np.zeros(B, dtype=np.int32),
                  None)
        if pr is None:
            return None
        preds, rows, lists = pr
        cur = torch.cuda.current_stream(self.device)
        live_only = len(preds) == 1 and tuple(
            preds.view(np.uint32)[0]) == pack_pred(None)
        if live_only and self._live_bits is not None:
            # cached until the next append or delete; the planes run on
            # different streams, so order this one after the producer
            bits, ready = self._live_bits
            cur.wait_event(ready)
            bits.record_stream(cur)
        elif lists is not None:
            desc, doms = self._list_tables(lists)
            bits = K.filter_bitmask_sets(
                self.attrs, torch.from_numpy(preds).to(self.device),
                torch.from_numpy(desc),
                torch.from_numpy(doms).to(self.device))
        else:
            bits = K.filter_bitmask(
                self.attrs, torch.from_numpy(preds).to(self.device))
            if live_only:
                ready = torch.cuda.Event()
                ready.record(cur)
                self._live_bits = (bits, ready)
        return bits, rows

    def hbm_bytes(self) -> int:
        total = sum(s.hbm_bytes() for s in self.segments)
        for t in (self._emb_buf, self._gid_buf, self._attr_buf,
                  self._dom_ws, *self._collapse_ws.values(),
                  *(self._dom_tables or ())):
            if t is not None:
                total += t.numel() * t.element_size()
        return total

    def _domain_tables(self) -> tuple[torch.Tensor, torch.Tensor]:
        """(dom_keys [D] i32, dom_id [N] i32) of this epoch: the distinct
        w2 words of the shard's rows, ascending as unsigned, and every
        row's index into them. Built on the device on first use."""
        if self._dom_tables is None:
            w2 = self.attrs[:, 2].long() & U32_MAX
            keys, inv = torch.unique(w2, return_inverse=True)
            keys = torch.where(keys > 0x7FFFFFFF, keys - (1 << 32), keys)
            self._dom_tables = (keys.to(torch.int32).contiguous(),
                                inv.to(torch.int32).contiguous())
        return self._dom_tables

    def _domain_ws(self, R: int, D: int) -> torch.Tensor:
        """[R, D] i32 view of the count workspace, grown on demand."""
        if self._dom_ws is None or self._dom_ws.numel() < R * D:
            self._dom_ws = torch.empty(R * D, device=self.device,
                                       dtype=torch.int32)
        return self._dom_ws[:R * D].view(R, D)

    def _collapse_rows(self, plane: str, scores: torch.Tensor, k: int,
                       caps: list[int], mask, vals: torch.Tensor,
                       idx: torch.Tensor) -> None:
        """Overwrite the capped rows of a plane's top-k (vals, idx
        [B, k]) with the first k of their capped sets, exact over the
        whole score row (ops/csrc/collapse.hip): domain_best x m and
        collapse_select over the scores and the mask the top-k read.
        plane: "bm25" (eligible: passes the mask and score > 0) or
        "dense" (passes the mask). Rows are grouped by m and taken in
        slices whose workspace stays within COLLAPSE_WS_BYTES."""
        from ..ops import kernels as K
        dom_keys, dom_id = self._domain_tables()
        D = dom_keys.numel()
        for m in sorted(set(caps) - {0}):
            rows = [b for b, c in enumerate(caps) if c == m]
            step = max(1, COLLAPSE_WS_BYTES // (m * D * 8))
            for lo in range(0, len(rows), step):
                part = rows[lo:lo + step]
                need = m * len(part) * D
                ws = self._collapse_ws.get(plane)
                if ws is None or ws.numel() < need:
                    ws = self._collapse_ws[plane] = torch.empty(
                        need, device=self.device, dtype=torch.int64)
                # one upload: the kernel's rows and the rows to overwrite
                rows_t = torch.tensor(part, dtype=torch.int32)
                rows_d = rows_t.to(self.device, non_blocking=True)
                best = K.domain_best(
                    scores, rows_t, dom_id, D, m, plane == "bm25",
                    out=ws[:need].view(m, len(part), D),
                    rows_device=rows_d, **_mask_kw(mask))
                c_vals, c_idx = K.collapse_select(best, k)
                at = rows_d.long()
                vals.index_copy_(0, at, c_vals)
                idx.index_copy_(0, at, c_idx.to(idx.dtype))

    def hit_domains(self, idx: torch.Tensor) -> torch.Tensor:
        """[B, k] shard-local columns (-1 pad) -> [B, k] i32 domain words
        (w2 of the attribute record), 0 at padding."""
        w2 = self.attrs[:, 2][idx.clamp(min=0).long()]
        return torch.where(idx >= 0, w2, torch.zeros_like(w2))

    # ----------------------------------------------------------- search
    def _get_topk(self):
        from ..ops.kernels import TopK
        if self._topk is None:
            self._topk = TopK(self.device)
        return self._topk

    def _get_topk_dense(self):
        """Separate selector (own workspace) so the dense plane can run
        on a different stream than the BM25 plane without racing."""
        from ..ops.kernels import TopK
        if self._topk_dense is None:
            self._topk_dense = TopK(self.device)
        return self._topk_dense

    def _idf(self, term: int) -> float:
        df = float(self.df[term])
        if df <= 0:
            return 0.0
        return math.log(1.0 + (self.n_docs - df + 0.5) / (df + 0.5))

    def _idf_table(self) -> np.ndarray:
        """Cached idf[V] f32 from the GLOBAL df (sum over segments)."""
        if self._h_idf is None:
            df = self.df.astype(np.float64)
            with np.errstate(divide="ignore"):
                idf = np.log(1.0 + (self.n_docs - df + 0.5) / (df + 0.5))
            self._h_idf = np.where(df > 0, idf, 0.0).astype(np.float32)
        return self._h_idf

    @staticmethod
    def dedupe_terms(queries_terms: list[np.ndarray]
                     ) -> tuple[np.ndarray, np.ndarray]:
        """Vectorized per-query term dedupe -> (qrows, terms), sorted by
        query row (the obvious per-query np.unique loop costs ~1 ms of
        host time at B=128, serializing the side-stream launch ahead of
        the encoder)."""
        B = len(queries_terms)
        if B == 0:
            return np.zeros(0, np.int64), np.zeros(0, np.int64)
        lens = np.fromiter((len(t) for t in queries_terms), np.int64, B)
        T = int(lens.max())
        if T == 0:
            return np.zeros(0, np.int64), np.zeros(0, np.int64)
        if (lens == lens[0]).all():
            mat = np.stack(queries_terms).astype(np.int64, copy=False)
        else:
            mat = np.full((B, T), -1, dtype=np.int64)
            for qi, t in enumerate(queries_terms):
                mat[qi, :len(t)] = t
        srt = np.sort(mat, axis=1)
        valid = srt >= 0
        valid[:, 1:] &= srt[:, 1:] != srt[:, :-1]
        qrows, cols = np.nonzero(valid)
        return qrows.astype(np.int64), srt[qrows, cols]

    def _pick_bd(self, B: int) -> int:
        """Doc-block size: 8K docs (32 KB LDS -> 5 workgroups/CU;
        measured 405 us vs 471/713 us for 16K/32K at 1.25M docs B=128,
        scripts/bm25_probe.py) unless that underfills the chip."""
        for bd in (8192, 4096):
            blocks = sum((s.n_docs + bd - 1) // bd for s in self.segments)
            if blocks * max(B, 1) >= 2048:
                return bd
        return 4096

    def _bounds_ws(self, n: int) -> torch.Tensor:
        """Device i32 workspace for the bounds pre-pass (reused across
        segments/batches; launches are stream-ordered so one suffices)."""
        ws = getattr(self, "_bounds_buf", None)
        if ws is None or ws.numel() < n:
            ws = self._bounds_buf = torch.empty(
                max(n, 1 << 16), device=self.device, dtype=torch.int32)
        return ws

    def _h2d(self, name: str, arr: np.ndarray,
             dtype: torch.dtype) -> torch.Tensor:
        """Stage a small host array through a persistent pinned buffer —
        pageable-memory copies block the host and defeat the side-stream
        overlap; pinned + non_blocking stays truly async."""
        t = torch.from_numpy(np.ascontiguousarray(arr)).to(dtype)
        if self.device.type != "cuda":
            return t
        pins = getattr(self, "_h2d_pins", None)
        if pins is None:
            pins = self._h2d_pins = {}
        n = t.numel()
        buf = pins.get(name)
        if buf is None or buf.numel() < n:
            buf = torch.empty(max(2 * n, 4096), dtype=dtype,
                              pin_memory=True)
            pins[name] = buf
        buf[:n].copy_(t)
        return buf[:n].to(self.device, non_blocking=True)

    def search_bm25(self, queries_terms: list[np.ndarray], k: int,
                    scores_buf: torch.Tensor | None = None,
                    mark=None, filters=None, _mask=None, term_ops=None,
                    per_domain=None
                    ) -> tuple[torch.Tensor, torch.Tensor]:
        """BM25 plane only (needs terms, not embeddings) — callable on a
        side stream to overlap with query encoding. One kernel launch
        per posting segment; the segments' disjoint doc ranges cover
        every column of the score matrix exactly once.

        filters: one DocFilter or None per query. With a filter in the
        batch or a tombstone in the shard the select is masked: the
        fused pass-1 histogram counts failing documents, so it is not
        produced and the masked top-k streams the matrix once more.
        term_ops: one TermOps or None per query; a row with operands
        selects among the documents that hold every required and no
        excluded term, and masks the batch like a filter does.
        per_domain: one int or None per query; a row with a cap m
        (1 .. COLLAPSE_M_MAX) returns at most m documents per domain,
        the first k of its capped set over the whole score row, in
        score order with ties by ascending column, bit for bit
        (ops/csrc/collapse.hip). Domains compare by their 32-bit hash,
        as filters and facets compare them: a hash collision can only
        over-collapse. The other rows are what they are without it."""
        return self._bm25_plane(queries_terms, k, scores_buf, mark, filters,
                                _mask, term_ops, None, per_domain)[:2]

    def search_bm25_top(self, queries_terms: list[np.ndarray], k: int,
                        facets, scores_buf: torch.Tensor | None = None,
                        mark=None, filters=None, _mask=None, term_ops=None,
                        per_domain=None):
        """search_bm25_facets plus the top domains of the rows that ask
        for them: -> (values, indices, counts, dom_top, dom_tally), the
        last two as ShardHits holds them (None when no row asks)."""
        return self._bm25_plane(queries_terms, k, scores_buf, mark, filters,
                                _mask, term_ops,
                                pack_facets(facets, len(queries_terms)),
                                per_domain)

    def search_bm25_facets(self, queries_terms: list[np.ndarray], k: int,
                           facets, scores_buf: torch.Tensor | None = None,
                           mark=None, filters=None, _mask=None,
                           term_ops=None, per_domain=None
                           ) -> tuple[torch.Tensor, torch.Tensor,
                                      torch.Tensor | None]:
        """search_bm25 that also counts facets over every matching
        document of the rows `facets` names (a FacetSpec or
        PackedFacets): -> (values, indices, counts [R, F] i32 or None
        when no row is counted). The count kernel (csrc/facets.hip) runs
        on this stream straight after the scores are written, over the
        buffer the top-k reads, with the same mask; it changes neither
        the mask nor the select, so an unmasked batch keeps the fused
        pass-1 histogram."""
        return self._bm25_plane(queries_terms, k, scores_buf, mark, filters,
                                _mask, term_ops,
                                pack_facets(facets, len(queries_terms)),
                                per_domain)[:3]

    def _bm25_plane(self, queries_terms, k, scores_buf, mark, filters,
                    _mask, term_ops, facets, per_domain=None):
        import time as _time
        from ..ops import kernels as K
        if mark is None:
            def mark(name, t0):
                return t0
        B = len(queries_terms)
        caps = per_domain_caps(per_domain, B)
        dev = self.device
        N = self.n_docs
        k = min(k, N)
        topk = self._get_topk()
        mask = _mask if _mask is not None else self._mask_for(filters, B,
                                                              term_ops)
        tp = _time.perf_counter()
        if scores_buf is not None and scores_buf.shape == (B, N):
            scores = scores_buf
        else:
            scores = torch.empty(B, N, device=dev, dtype=torch.float32)
        qrows, terms = self.dedupe_terms(queries_terms)
        # queries share Zipf-common terms: dedupe ACROSS queries so the
        # bounds pre-pass searches each term's postings once per block
        uterms, qt_ut = np.unique(terms, return_inverse=True)
        idf = self._idf_table()[terms]
        qt_off = np.zeros(B + 1, dtype=np.int64)
        np.cumsum(np.bincount(qrows, minlength=B), out=qt_off[1:])
        bd = self._pick_bd(B)
        U = len(uterms)
        # Unmasked batch, every segment starting at a multiple of 64 (a
        # 64-column block then lies in one segment): the block kernel
        # also writes each block's maximum and the select reads those
        # and k blocks per row, never [B, N]. A mask would have to keep
        # failing documents out of the maxima.
        pruned = (mask is None and self.bm25_pruned and dev.type == "cuda"
                  and all(s.doc_base % 64 == 0 for s in self.segments))
        bmax = hist = None
        if pruned:
            bmax = self._bm25_bmax.get(B)
            if bmax is None or bmax.shape != (B, (N + 63) // 64):
                bmax = self._bm25_bmax[B] = torch.empty(
                    B, (N + 63) // 64, device=dev, dtype=torch.float32)
        elif mask is None:
            # fused topk pass 1: the block kernel histograms every score
            # it writes, so the top-k select skips one full read of the
            # [B, N] array (~0.9 ms/batch at 10M docs)
            hists = getattr(self, "_bm25_hists", None)
            if hists is None:
                hists = self._bm25_hists = {}
            hist = hists.get(B)
            if hist is None:
                hist = hists[B] = torch.zeros(
                    B * 256, device=dev, dtype=torch.int32)
            else:
                hist.zero_()
        tp = mark("shard.chunks", tp)
        # don't overwrite the pinned staging buffers while a prior
        # step's async H2D copy could still be in flight
        evt = getattr(self, "_h2d_evt", None)
        if evt is not None:
            evt.synchronize()
        qt_off_d = self._h2d("qt_off", qt_off, torch.int32)
        qt_ut_d = self._h2d("qt_ut", qt_ut, torch.int32)
        qt_idf_d = self._h2d("qt_idf", idf, torch.float32)
        for si, seg in enumerate(self.segments):
            nblocks = (seg.n_docs + bd - 1) // bd
            bounds = self._bounds_ws(U * nblocks * 2)
            K.bm25_block(
                seg.doc_ids, seg.tfdl, qt_off_d, qt_ut_d, qt_idf_d,
                self._h2d(f"qb{si}", seg.h_offs[uterms], torch.int64),
                self._h2d(f"qe{si}", seg.h_offs[uterms + 1], torch.int64),
                bounds, scores, seg.doc_base, seg.n_docs, bd,
                self.avgdl, k1=BM25_K1, b=BM25_B,
                hist1=hist, bmax=bmax)
        if dev.type == "cuda":
            if evt is None:
                evt = self._h2d_evt = torch.cuda.Event()
            evt.record()
        tp = mark("shard.bm25", tp)
        counts = None
        if facets is not None:
            rows_t, edges_t, langs_t, desc_t, doms_t = (
                torch.from_numpy(t) for t in facets.tables())
            counts = K.facet_counts(
                scores, rows_t, self.attrs, edges_t, langs_t, desc_t,
                doms_t, **_mask_kw(mask))
            tp = mark("shard.facets", tp)
        dom_top = tally = None
        if facets is not None and facets.top_rows:
            # the same scores and the same mask once more, 4 bytes per
            # match: the tally by domain id, then its first entries
            dom_keys, dom_id = self._domain_tables()
            top_rows = torch.tensor(facets.top_rows, dtype=torch.int32)
            D = dom_keys.numel()
            cnt = K.domain_count(
                scores, top_rows, dom_id, D,
                out=self._domain_ws(len(facets.top_rows), D),
                **_mask_kw(mask))
            dom_top = K.domain_select(cnt, dom_keys, TOP_FETCH + 1)
            tally = DomainTally(cnt, dom_keys)
            tp = mark("shard.topdomains", tp)
        if pruned:
            if self._topk_pruned_bm25 is None:
                self._topk_pruned_bm25 = K.TopKPruned(dev)
            out = self._topk_pruned_bm25(scores, bmax, 64, k)
        elif mask is None:
            out = topk(scores, k, ext_hist1=hist)
        else:
            out = topk(scores, k, mask=mask[0], row_pred=mask[1])
        tp = mark("shard.bm25topk", tp)
        if caps is not None:
            self._collapse_rows("bm25", scores, k, caps, mask, out[0],
                                out[1])
            mark("shard.bm25collapse", tp)
        self._bm25_scores_buf = scores
        return out[0], out[1], counts, dom_top, tally

    def search(self, queries_terms: list[np.ndarray],
               query_emb: torch.Tensor | None, k: int = 100,
               scores_buf: torch.Tensor | None = None,
               phase_t: dict | None = None,
               filters: list[DocFilter | None] | None = None,
               term_ops: list[TermOps | None] | None = None,
               facets: FacetSpec | None = None,
               per_domain: list[int | None] | None = None) -> ShardHits:
        """Score all queries against this shard; returns fixed-size
        top-k with global ids (the per-peer result cap analogue,
        reference p2p/routing.py:48). filters: one DocFilter or None per
        query; filtered-out and deleted documents are never returned,
        and a row with fewer than k passing documents pads with
        -inf / id -1. term_ops: one TermOps or None per query; both
        planes return only documents that hold every required and no
        excluded term (a required id that is nowhere in the shard
        leaves the row all padding). facets: a FacetSpec (or
        PackedFacets); ShardHits.facets then holds the counts over every
        matching document of the rows it names, and the hits are what
        they are without it. per_domain: one int or None per query, as
        in search_bm25; both planes of a capped row return at most m
        documents per domain (the dense plane over every document that
        passes the mask), and ShardHits.bm25_dom / dense_dom hold the
        hits' domain words."""
        import time as _time

        def mark(name, t0):
            if phase_t is None:
                return t0
            torch.cuda.synchronize()
            t1 = _time.perf_counter()
            phase_t[name] = phase_t.get(name, 0.0) + (t1 - t0)
            return t1

        B = len(queries_terms)
        N = self.n_docs
        dev = self.device
        assert N > 0, "shard is empty"
        k = min(k, N)
        tp = _time.perf_counter()
        mask = self._mask_for(filters, B, term_ops)   # once for both planes
        counts = dom_top = tally = None
        if facets is None:
            bm_vals, bm_idx = self.search_bm25(queries_terms, k,
                                               scores_buf=scores_buf,
                                               mark=mark, _mask=mask,
                                               per_domain=per_domain)
        else:
            bm_vals, bm_idx, counts, dom_top, tally = self.search_bm25_top(
                queries_terms, k, facets, scores_buf=scores_buf, mark=mark,
                _mask=mask, per_domain=per_domain)
        tp = _time.perf_counter()

        # --- dense plane ---
        if query_emb is not None and self.embeddings is not None:
            dn_vals, dn_idx = self.search_dense(query_emb, k, mark=mark,
                                                _mask=mask,
                                                per_domain=per_domain)
        else:
            dn_vals = torch.full((B, k), -float("inf"), device=dev)
            dn_idx = torch.full((B, k), -1, device=dev, dtype=torch.int32)

        return ShardHits(bm25_scores=bm_vals,
                         bm25_ids=self.to_global(bm_idx),
                         dense_scores=dn_vals,
                         dense_ids=self.to_global(dn_idx), facets=counts,
                         dom_top=dom_top, dom_tally=tally,
                         **self._hit_dom_fields(per_domain, B, bm_idx,
                                                dn_idx))

    def _hit_dom_fields(self, per_domain, B: int, bm_idx, dn_idx) -> dict:
        """ShardHits' bm25_dom / dense_dom of a batch with a capped row;
        nothing otherwise."""
        if per_domain_caps(per_domain, B) is None:
            return {}
        return {"bm25_dom": self.hit_domains(bm_idx),
                "dense_dom": self.hit_domains(dn_idx)}

    def search_dense(self, query_emb: torch.Tensor, k: int,
                     mark=None, filters=None, _mask=None, term_ops=None,
                     per_domain=None
                     ) -> tuple[torch.Tensor, torch.Tensor]:
        """Dense (cosine) plane; runs after the query embedding exists.
        filters, term_ops, per_domain: as in search_bm25, with every
        document that passes the mask eligible, whatever its score. The
        collapse kernels read the plane's score buffer after the top-k,
        outside the captured graph: the buffer still holds the batch's
        scores when a graph has replayed."""
        import time as _time
        from ..ops import kernels as K
        if mark is None:
            def mark(name, t0):
                return t0
        B = query_emb.shape[0]
        N = self.n_docs
        k = min(k, N)
        mask = _mask if _mask is not None else self._mask_for(filters, B,
                                                              term_ops)
        caps = per_domain_caps(per_domain, B)
        tp = _time.perf_counter()
        emb = self.embeddings
        # hipGraph capture of the whole plane (GEMM + top-k passes, all
        # fixed shapes) removes ~10 launch gaps per batch. Opt-in per
        # shard (graph_dense). Graphs are invalidated on every append
        # (the captured embeddings view goes stale).
        # A masked batch runs uncaptured: its mask and row_pred tensors
        # change per batch, which a captured graph cannot follow.
        if self.device.type == "cuda" and self.graph_dense and mask is None:
            g = self._dense_graphs.get((B, k))
            if g is None:
                from ..ops.graphs import GraphedCallable

                # A selector of its own per graph: replays keep writing
                # the workspace recorded at capture, which a selector
                # shared across batch sizes would free when it regrows.
                def _plane(e, _B=B, _k=k, _emb=emb,
                           _tk=(K.TopK(self.device),
                                K.TopKPruned(self.device))):
                    return self._dense_select(
                        self._dense_gemm(e, _emb, _B, self.n_docs), _k, *_tk)
                g = self._dense_graphs[(B, k)] = GraphedCallable(_plane)
            vals, idx = g(query_emb.bfloat16())
            # detach from the graph's static outputs (next replay
            # overwrites them)
            out = (vals.clone(), idx.clone())
            tp = mark("shard.dense+topk", tp)
            if caps is not None:
                self._collapse_rows(
                    "dense", self._get_dense_buf(B).reshape(B, N), k, caps,
                    None, *out)
                mark("shard.densecollapse", tp)
            return out
        d_scores = self._dense_gemm(query_emb, emb, B, N,
                                    with_bmax=mask is None)
        tp = mark("shard.dense", tp)
        if mask is None:
            if self._topk_pruned is None:
                self._topk_pruned = K.TopKPruned(self.device)
            out = self._dense_select(d_scores, k, self._get_topk_dense(),
                                     self._topk_pruned)
        else:
            out = self._get_topk_dense()(d_scores, k, mask=mask[0],
                                         row_pred=mask[1])
        tp = mark("shard.densetopk", tp)
        if caps is not None:
            self._collapse_rows(
                "dense", self._get_dense_buf(B).reshape(B, N), k, caps, mask,
                *out)
            mark("shard.densecollapse", tp)
        return out

    @staticmethod
    def _dense_select(d_scores, k: int, topk, topk_pruned):
        """Top-k of what _dense_gemm returned: from the block maxima
        when it wrote them, else the streaming selector."""
        if isinstance(d_scores, tuple):
            return topk_pruned(*d_scores, k)
        return topk(d_scores, k)

    def _dense_gemm(self, query_emb: torch.Tensor, emb: torch.Tensor,
                    B: int, N: int, with_bmax: bool = True):
        """Dense cosine scores [B, N] on the stored-embedding dtype:
        bf16 -> generic MFMA tile; fp8 -> streaming fp8 kernel (M
        chunks of <=128; query quantized per batch).
        with_bmax (unmasked batches; a mask would have to keep failing
        documents out of the maxima): on the bf16 plane, where the GEMM
        has the variant for this shape, returns (scores, bmax, W) with
        the block maxima for the pruned selector."""
        from ..ops import kernels as K
        buf = self._get_dense_buf(B)
        if self.emb_dtype == "fp8":
            qa = query_emb
            if qa.dtype != torch.float8_e4m3fn:
                qa = qa.float().to(torch.float8_e4m3fn)
            out2d = buf.reshape(B, N)
            for m0 in range(0, B, 128):
                m1 = min(m0 + 128, B)
                r = K.dense_scores_fp8(qa[m0:m1].contiguous(), emb,
                                       out=out2d[m0:m1])
                assert r is not None, "fp8 dense plane shape ineligible"
            return out2d
        W = K.gemm_bmax_width(B, N, emb.shape[1]) if with_bmax else 0
        if W:
            bmax = self._dense_bmax.get(B)
            if bmax is None or bmax.shape != (B, (N + W - 1) // W):
                # per B and dropped with the score buffers, for the
                # reason given in _get_dense_buf
                bmax = self._dense_bmax[B] = torch.empty(
                    B, (N + W - 1) // W, device=self.device,
                    dtype=torch.float32)
            return K.gemm_nt_bmax(query_emb.bfloat16().contiguous(), emb,
                                  out=buf.reshape(B, N), bmax=bmax)
        return K.gemm_nt(query_emb.bfloat16().unsqueeze(0), emb,
                         out_f32=True, out=buf).reshape(B, N)

    def _get_dense_buf(self, B: int) -> torch.Tensor:
        """Persistent dense scores buffer, separate from the BM25 one
        (which may still be feeding its top-k on another stream). Keyed
        per batch size: captured hipGraphs keep writing the buffer they
        recorded, so a shared buffer reallocated for a different B
        would leave older graphs writing freed memory (the serving
        batcher sends pow2-bucketed batch sizes, so this cache is
        bounded). Reuse avoids a multi-GB alloc/free per batch."""
        N = self.n_docs
        bufs = getattr(self, "_dense_bufs", None)
        if bufs is None:
            bufs = self._dense_bufs = {}
        buf = bufs.get(B)
        if buf is None or buf.shape != (1, B, N):
            buf = bufs[B] = torch.empty(
                1, B, N, device=self.device, dtype=torch.float32)
        return buf

    def to_global(self, idx: torch.Tensor) -> torch.Tensor:
        safe = idx.clamp(min=0).long()
        g = self.global_ids[safe]
        return torch.where(idx >= 0, g, torch.full_like(g, -1))


class CpuShard(GpuShard):
    """CPU shard with identical semantics, scored by plain torch/numpy.

    Used on machines without a GPU (tests, the CPU-plumbing config, and
    multi-process gloo tests of the query plane). On a GPU box the HIP
    path is always taken — this class is never a silent GPU fallback."""

    def __init__(self, vocab: int = BM25_VOCAB, emb_dtype: str = "bf16"):
        super().__init__(device="cpu", vocab=vocab, emb_dtype=emb_dtype)

    def _holds(self, term: int) -> np.ndarray:
        """bool [N]: the documents with a posting for this term id."""
        has = np.zeros(self.n_docs, dtype=bool)
        for seg in self.segments:
            b, e = int(seg.h_offs[term]), int(seg.h_offs[term + 1])
            has[seg.doc_ids.numpy()[b:e].astype(np.int64) + seg.doc_base] = True
        return has

    def _fail_rows(self, filters, B: int,
                   term_ops=None) -> torch.Tensor | None:
        """bool [B, N], True where a document fails its row's predicate
        (the same packed words the GPU kernel reads) or its row's term
        operands (a required term it lacks, an excluded one it holds);
        None when the mask is inactive."""
        pr = self._pred_rows(filters, B)
        trows = self._term_rows(term_ops, B)
        if pr is None and not trows:
            return None
        if pr is None:
            fail = np.zeros((B, self.n_docs), dtype=bool)
        else:
            preds, rows, lists = pr
            a = self.attrs.numpy()
            if lists is None:
                lists = [((), ())] * len(preds)
            ok = np.stack([passes(a, p, allow=allow, block=block)
                           for p, (allow, block) in zip(preds.view(np.uint32),
                                                        lists)])
            fail = ~ok[rows]
        for i, t in trows:
            for term in t.require:
                fail[i] |= ~self._holds(term)
            for term in t.exclude:
                fail[i] |= self._holds(term)
        return torch.from_numpy(fail)

    @staticmethod
    def _masked_topk(scores: torch.Tensor, fail: torch.Tensor | None,
                     k: int) -> tuple[torch.Tensor, torch.Tensor]:
        if fail is None:
            return torch.topk(scores, k, dim=1)
        vals, idx = torch.topk(
            scores.masked_fill(fail, -float("inf")), k, dim=1)
        return vals, torch.where(vals == -float("inf"),
                                 torch.full_like(idx, -1), idx)

    def search(self, queries_terms, query_emb, k: int = 100,
               scores_buf=None, phase_t=None, filters=None,
               term_ops=None, facets=None, per_domain=None) -> ShardHits:
        B = len(queries_terms)
        N = self.n_docs
        assert N > 0, "shard is empty"
        k = min(k, N)
        norm = self.doc_norm.numpy()
        scores = np.zeros((B, N), dtype=np.float32)
        for seg in self.segments:
            offs = seg.h_offs
            doc_ids = seg.doc_ids.numpy()
            tfdl = seg.tfdl.numpy().view(np.uint32)
            tf_all = (tfdl & np.uint32(0xFFFF)).astype(np.float32)
            for qi, terms in enumerate(queries_terms):
                for t in np.unique(terms):
                    t = int(t)
                    b, e = int(offs[t]), int(offs[t + 1])
                    if b == e:
                        continue
                    idf = self._idf(t)
                    d = doc_ids[b:e].astype(np.int64) + seg.doc_base
                    tf = tf_all[b:e]
                    scores[qi, d] += (idf * tf * (BM25_K1 + 1)
                                      / (tf + norm[d]))
        st = torch.from_numpy(scores)
        fail = self._fail_rows(filters, B, term_ops)
        bm_vals, bm_idx = self._masked_topk(st, fail, k)
        caps = per_domain_caps(per_domain, B)
        self._collapse_rows_np(st, k, caps, fail, True, bm_vals, bm_idx)
        counts = dom_top = tally = None
        packed = pack_facets(facets, B)
        if packed is not None:
            fail_np = None if fail is None else fail.numpy()
            counts = torch.from_numpy(facet_counts_np(
                scores, fail_np, self.attrs.numpy(), packed))
            if packed.top_rows:
                dom_top = torch.from_numpy(domain_top_np(
                    scores, fail_np, self.attrs.numpy(), packed.top_rows,
                    TOP_FETCH + 1))
                dom_keys, dom_id = self._domain_tables()
                D = dom_keys.numel()
                cnt = self._domain_ws(len(packed.top_rows), D)
                for r, b in enumerate(packed.top_rows):
                    m = scores[b] > 0
                    if fail_np is not None:
                        m &= ~fail_np[b]
                    cnt[r] = torch.from_numpy(np.bincount(
                        dom_id.numpy()[m], minlength=D).astype(np.int32))
                tally = DomainTally(cnt, dom_keys)
        if query_emb is not None and self.embeddings is not None:
            d_scores = query_emb.float().cpu() @ self.embeddings.float().T
            dn_vals, dn_idx = self._masked_topk(d_scores, fail, k)
            self._collapse_rows_np(d_scores, k, caps, fail, False, dn_vals,
                                   dn_idx)
        else:
            dn_vals = torch.full((B, k), -float("inf"))
            dn_idx = torch.full((B, k), -1, dtype=torch.int64)

        def to_global(idx):
            safe = idx.clamp(min=0).long()
            g = self.global_ids[safe]
            return torch.where(idx >= 0, g, torch.full_like(g, -1))

        return ShardHits(bm25_scores=bm_vals, bm25_ids=to_global(bm_idx),
                         dense_scores=dn_vals.float(),
                         dense_ids=to_global(dn_idx), facets=counts,
                         dom_top=dom_top, dom_tally=tally,
                         **self._hit_dom_fields(per_domain, B, bm_idx,
                                                dn_idx))

    def _collapse_rows_np(self, scores: torch.Tensor, k: int, caps, fail,
                          positive: bool, vals, idx) -> None:
        """GpuShard._collapse_rows through the oracle
        (ops/reference.collapse_topk_rows), row by row."""
        if caps is None:
            return
        from ..ops.reference import collapse_topk_rows
        dom_id = self._domain_tables()[1]
        fail_np = None if fail is None else fail.numpy()
        for b, m in enumerate(caps):
            if m:
                v, i = collapse_topk_rows(
                    scores[b:b + 1].float(),
                    None if fail_np is None else fail_np[b:b + 1], dom_id,
                    [0], m, k, positive)
                vals[b] = v[0].to(vals.dtype)
                idx[b] = i[0].to(idx.dtype)

    def _domain_tables(self) -> tuple[torch.Tensor, torch.Tensor]:
        """GpuShard's tables, built with numpy."""
        if self._dom_tables is None:
            self._dom_tables = tuple(
                torch.from_numpy(t)
                for t in domain_tables_np(self.attrs.numpy()))
        return self._dom_tables
