"""Service orchestration: AppContext wiring + the crawl->index->publish
and search entry paths.

Reference parity: infomesh/services.py (AppContext role-conditional
construction, index_document single source of truth, crawl_and_index,
fetch_page cache-first, create_local_search_fn). The network-publish
path becomes a GPU-engine ingest (SURVEY.md §2.9 last row).
"""
from __future__ import annotations

import logging
import math
import time
from collections import Counter
from dataclasses import dataclass, field
from typing import Any

from .config import Config, load_config
from .credits.farming import FarmingDetector
from .credits.ledger import Action, CreditLedger
from .crawler.dedup import DeduplicatorDB
from .crawler.robots import RobotsChecker
from .crawler.rss import FeedMonitor
from .crawler.scheduler import Scheduler
from .crawler.worker import CrawlResult, CrawlWorker
from .engine import HybridEngine
from .errors import GpuExtensionMissing, InfoMeshError
from .crawler.lang_detect import known_languages
from .index.doc_attrs import (FACET_MAX_DOMS, TOP_DOMAINS_MAX, DocFilter,
                              FacetCounts, FacetSpec, pack_pred_sets)
from .index.gpu_index import bm25_term_ids, per_domain_caps
from .index.link_graph import LinkGraph
from .index.local_store import Document, LocalStore
from .search.batcher import QueryBatcher
from .search.cache import QueryCache
from .search.facets import compute_facets
from .search.nlp import (RelatedSearchTracker, parse_facet_request,
                         parse_facet_token, parse_persite_token,
                         parse_query_filters, parse_term_operators,
                         with_facet_request, with_filter_tokens,
                         with_persite_token)
from .search.passage import fast_snippet
from .search.query import (SearchResponse, preprocess_query,
                           search_hybrid, search_local)
from .trust.attestation import create_attestation
from .trust.dmca import TakedownManager
from .trust.gdpr import DeletionManager
from .trust.keys import KeyPair, ensure_keys
from .trust.scoring import TrustStore

log = logging.getLogger("infomesh.services")

# The shards hash words into 2^17 term ids; the hydration guard for
# required words compares the same tokens hashed into 2^62, where two
# words do not meet in practice.
_GUARD_VOCAB = 1 << 62

# date facet: the reference's labels (infomesh/search/facets.py), oldest
# first, as the buckets between the edges floor(now) - {365, 30, 7, 1}
# days and floor(now) + 1 come out; a crawl time of 0 and one in the
# future are both "unknown"
_DATE_LABELS = ("older", "this_year", "this_month", "this_week", "today",
                "unknown")
_DATE_AGES_D = (365, 30, 7, 1)


@dataclass
class FacetedHits:
    """What _batch_execute returns for a query that carried a facet
    token: its hydrated hits (cut to the batch's limit, not the
    caller's) and its counts over the whole match set."""
    hits: list
    counts: FacetCounts | None


@dataclass
class AppContext:
    """All wired subsystems for one node process.

    Role-conditional (reference services.py:485-567): 'crawler' skips
    the query cache + engine; 'search' skips the crawl worker."""

    config: Config
    store: LocalStore
    link_graph: LinkGraph
    dedup: DeduplicatorDB
    keys: KeyPair
    ledger: CreditLedger
    trust: TrustStore
    takedowns: TakedownManager
    deletions: DeletionManager
    cache: QueryCache
    feeds: FeedMonitor
    related: RelatedSearchTracker
    feedback: object | None = None
    worker: CrawlWorker | None = None
    engine: HybridEngine | None = None
    batcher: QueryBatcher | None = None
    recrawl_queue: Any = None   # crawler.freshness.PriorityRecrawlQueue
    attestations: list = field(default_factory=list)
    farming: FarmingDetector = field(default_factory=FarmingDetector)
    started_at: float = field(default_factory=time.time)
    # resource ladder: crawl loop consults it for backpressure and
    # index_document refuses writes at READ_ONLY (reference
    # governor.py:49-74 semantics)
    governor: Any = None
    otlp: Any = None   # utils.observability.OtlpExporter (off by default)
    # the engine's hash -> domain name map was refilled from the store
    # (_domain_label does it once, on the first unknown hash)
    _domain_names_loaded: bool = False

    # ------------------------------------------------------------ build
    @classmethod
    def create(cls, config: Config | None = None,
               with_engine: bool | None = None,
               with_worker: bool | None = None,
               in_memory: bool = False) -> "AppContext":
        cfg = config or load_config()
        role = cfg.node.role
        data = cfg.data_dir
        if not in_memory:
            data.mkdir(parents=True, exist_ok=True)

        def p(name: str):
            return ":memory:" if in_memory else data / name

        if cfg.node.plugins:
            from .utils.plugins import load_plugins_from_config
            load_plugins_from_config(
                [x.strip() for x in cfg.node.plugins.split(",")
                 if x.strip()])
        store = LocalStore(p("index.db"), tokenizer=cfg.index.fts_tokenizer,
                           max_text_chars=cfg.index.max_text_chars)
        keys = KeyPair.generate() if in_memory else ensure_keys(data)
        ledger = CreditLedger(p("ledger.db"), kp=keys,
                              crawl_reward=cfg.credits.crawl_reward,
                              query_reward=cfg.credits.query_reward,
                              search_cost=cfg.credits.search_cost,
                              grace_hours=cfg.credits.grace_hours)
        trust = TrustStore(p("trust.db"),
                           isolation_failures=cfg.trust.isolation_failures)
        ctx = cls(
            config=cfg,
            store=store,
            link_graph=LinkGraph(p("links.db")),
            dedup=DeduplicatorDB(p("dedup.db")),
            keys=keys,
            ledger=ledger,
            trust=trust,
            takedowns=TakedownManager(store, keys, p("dmca.db")),
            deletions=DeletionManager(store, keys, p("gdpr.db")),
            cache=QueryCache(cfg.search.cache_entries, cfg.search.cache_ttl_s),
            feeds=FeedMonitor(path=None if in_memory else p("feeds.json")),
            related=RelatedSearchTracker(),
        )
        # GDPR / DMCA deletions reach the GPU engine at once (the
        # engine may be attached later, so the hook looks it up)
        ctx.deletions.on_delete = ctx._engine_forget
        ctx.takedowns.on_delete = ctx._engine_forget
        from .search.feedback import FeedbackStore
        ctx.feedback = FeedbackStore(p("feedback.db"))
        from .utils.governor import ResourceGovernor
        ctx.governor = ResourceGovernor()
        if cfg.api.otlp_endpoint:
            from .utils.observability import OtlpExporter
            ctx.otlp = OtlpExporter(endpoint=cfg.api.otlp_endpoint)
        if with_worker if with_worker is not None else role in ("full", "crawler"):
            ctx.worker = CrawlWorker(
                cfg.crawl,
                scheduler=Scheduler(cfg.crawl.politeness_delay_s,
                                    cfg.crawl.max_urls_per_hour,
                                    cfg.crawl.max_depth),
                dedup=ctx.dedup,
                robots=RobotsChecker(cfg.crawl.user_agent))
        want_engine = with_engine if with_engine is not None \
            else role in ("full", "search")
        if want_engine:
            try:
                ctx.engine = HybridEngine(
                    k_per_shard=cfg.gpu.topk_per_shard,
                    emb_dtype="fp8" if cfg.gpu.dtype == "fp8" else "bf16",
                    hbm_budget_gb=cfg.gpu.hbm_budget_gb,
                    embed_max_chars=cfg.index.embed_max_chars,
                    require_extension=cfg.gpu.require_extension)
            except GpuExtensionMissing:
                # gpu.require_extension means FAIL, not degrade: a GPU
                # node silently serving the CPU path is exactly what
                # the knob exists to prevent
                raise
            except Exception as e:
                log.warning("engine unavailable: %s", e)
        if ctx.engine is not None:
            # all entry points share one micro-batching queue so
            # concurrent requests reach the GPU plane as one batch;
            # hydration happens batch-wide inside the executor (one
            # SQLite IN query per batch, fast snippets)
            ctx.batcher = QueryBatcher(
                ctx.engine, max_batch=cfg.search.batch_max,
                max_wait_ms=cfg.search.batch_wait_ms,
                execute=ctx._batch_execute)
        return ctx

    # ------------------------------------------------------------ ingest
    def index_document(self, doc: Document, attest: bool = True,
                       credit: bool = True) -> int | None:
        """THE single crawl->index source of truth
        (reference: services.py:68-110)."""
        from .utils.plugins import GLOBAL_PLUGINS
        if self.governor is not None and not self.governor.writes_allowed():
            raise InfoMeshError(
                "RT002", "node degraded to read-only (resource governor)")
        doc = GLOBAL_PLUGINS.run("pre_index", doc)
        if self.deletions.is_forgotten(doc.url):
            raise InfoMeshError("SEC001", "url under GDPR deletion record")
        if self.takedowns.is_blocked(doc.url):
            raise InfoMeshError("SEC001", "url under DMCA takedown")
        rowid = self.store.add_document(doc)
        if rowid is None:
            return None
        doc.doc_id = rowid
        if self.engine is not None:
            self.engine.add_document(doc)
        if attest:
            # deferred signature: signing eagerly cost ~3 ms/page of
            # pure-python Ed25519 on the hot ingest path for a
            # write-mostly log; signed_attestations() completes them
            # on first serve
            self.attestations.append(create_attestation(
                self.keys, doc.url, doc.raw_hash, doc.text_hash,
                sign=False))
            if len(self.attestations) > 10_000:
                del self.attestations[:5000]
        if credit:
            if self.farming.multiplier() > 0:
                # batched: one signed ledger entry per flush interval
                # (another ~3 ms/page of Ed25519 off the ingest path)
                self.ledger.record_action_async(Action.CRAWL, 1.0)
            self.farming.record("crawl")
        self.cache.invalidate()
        GLOBAL_PLUGINS.run("post_index", doc, rowid=rowid)
        return rowid

    def _engine_forget(self, doc_ids: list[int]) -> int:
        """Deletion hook of the GDPR / DMCA managers: tombstone the
        rows on the GPU plane (no flush needed) and drop cached
        responses that may still list them."""
        self.cache.invalidate()
        if self.engine is None:
            return 0
        return self.engine.delete_documents(doc_ids)

    def signed_attestations(self, limit: int = 100) -> list:
        """Serve the newest attestations, completing any deferred
        signatures (reference: attestations published to peers/DHT)."""
        from .trust.attestation import sign_attestation
        out = self.attestations[-limit:]
        for att in out:
            sign_attestation(self.keys, att)
        return out

    async def crawl_and_index(self, url: str, depth: int = 0,
                              force: bool = False) -> dict[str, Any]:
        """Crawl one URL and index it (reference: services.py:354-423)."""
        if self.worker is None:
            raise InfoMeshError("RT001", "no crawl worker in this role")
        from .utils.plugins import GLOBAL_PLUGINS
        url = GLOBAL_PLUGINS.run("pre_crawl", url)
        doc_meta = self.store.get_document_by_url(url)
        res: CrawlResult = await self.worker.crawl_url(
            url, depth=depth, force=force,
            etag=doc_meta.etag if doc_meta else "",
            last_modified=doc_meta.last_modified if doc_meta else "")
        out: dict[str, Any] = {"url": url, "status": res.status,
                               "reason": res.reason}
        if res.not_modified:
            self.store.update_recrawl(url, changed=False)
            return out
        if res.status != "ok" or res.page is None:
            return out
        page = res.page
        self.link_graph.add_links(url, page.links)
        for f in res.feeds:
            self.feeds.add(f)
        doc = Document(url=url, title=page.title, text=page.text,
                       language=page.language, text_hash=page.text_hash,
                       raw_hash=page.raw_html_hash, etag=res.etag,
                       last_modified=res.last_modified)
        rowid = self.index_document(doc)
        if doc_meta is not None:
            self.store.update_recrawl(url, changed=rowid is not None,
                                      etag=res.etag,
                                      last_modified=res.last_modified)
        out.update({"doc_id": rowid, "title": page.title,
                    "links": page.links[:50],
                    "links_scheduled": res.links_scheduled,
                    "indexed": rowid is not None})
        return GLOBAL_PLUGINS.run("post_crawl", out)

    # ------------------------------------------------------------ search
    def search(self, query: str, limit: int | None = None,
               mode: str = "auto", use_cache: bool = True,
               deduct: bool = True, include_domains=None,
               exclude_domains=None,
               recency_days: float = 0, facets: bool = False,
               facet_domains=(), top_domains: int = 0,
               per_domain: int = 0) -> SearchResponse:
        """Unified search entry (reference mcp/handlers.py:382 flow):
        cache -> credits -> local/hybrid/distributed -> cache.

        include_domains / exclude_domains: exact stored domains to
        allow / block (the reference's include_domains / exclude_domains);
        recency_days: only documents crawled that recently, to the
        minute. All three travel as filter tokens in the query text, so
        they reach the cache key and whichever path serves the query.
        On the GPU plane one query's lists hold at most
        doc_attrs.MAX_LIST_HASHES domains; more is a ValueError.

        facets: also fill SearchResponse.total_matches and .facets.
        Served by the engine, the counts cover EVERY document that
        matches the query (passes its filters and operators and holds a
        query term), on all shards: "scope": "matches", languages as
        crawler/lang_detect knows them plus "unknown" and "other",
        date_ranges by the reference's labels, and domains for the
        names in facet_domains only (at most doc_attrs.FACET_MAX_DOMS,
        more is a ValueError; they count by 32-bit hash). Served from
        FTS, the counts cover the returned hits ("scope": "results")
        and total_matches is None. A request without facets gets the
        response it always got.

        top_domains (with facets): T > 0 adds "top_domains" to the
        facets, {name: count} of the first T domains of the whole match
        set by count, then by 32-bit hash; at most
        doc_attrs.TOP_DOMAINS_MAX, more is a ValueError. The counts are
        exact over all shards. "top_domains_exact" says whether the T
        names are surely the true first T; when it is False a domain
        that is not shown may hold up to "top_domains_bound" matches.
        A hash whose name is unknown reads "#%08x". Served from FTS it
        is the hits' most common T domains, without those two keys.

        per_domain: m > 0 returns at most m hits per site, 1 <= m <= 4;
        a persite:N token typed into the query asks for the same, and
        the parameter wins. Outside the range is a ValueError, here, on
        the caller's thread. Served by the engine, the cap is exact over
        the whole match set: every shard picks each site's best m on
        both planes, and the fused list is capped again, so up to
        `limit` hits of different sites come back. Sites compare by
        32-bit hash there: two sites whose hashes collide share one cap.
        Served from FTS, the hit list is thinned by quality.diversify's
        greedy rule, with the hits over the cap dropped: the cap then
        covers the returned hits only, which can leave fewer than
        `limit`."""
        from .utils.plugins import GLOBAL_PLUGINS
        query = GLOBAL_PLUGINS.run("pre_search", query, mode=mode)
        # persite:N is split off on the caller's thread (a bad N fails
        # this caller alone); _engine_search writes it back for the
        # batch, the FTS paths never see it
        query, typed = parse_persite_token(query)
        cap = int(per_domain or 0) or typed
        per_domain_caps([cap], 1)           # out of range: a ValueError
        # facets:@... is the serving path's own syntax (_engine_search
        # writes it, _batch_execute reads it): one typed into the query
        # is dropped here, on the caller's thread, so that it neither
        # asks for counts nobody reads nor reaches the shared batch.
        # Facets are asked for with the `facets` parameter.
        query = parse_facet_token(query)[0]
        if include_domains or exclude_domains or recency_days:
            after = None
            if recency_days:
                # whole minutes, so that repeats of a query share a key
                after = (time.time() - float(recency_days) * 86400) // 60 * 60
            query = with_filter_tokens(query, include_domains,
                                       exclude_domains, after)
        limit = limit or self.config.search.max_results
        fdoms = None
        top = int(top_domains or 0) if facets else 0
        if top < 0 or top > TOP_DOMAINS_MAX:
            raise ValueError(
                f"top_domains = {top}; the cap is {TOP_DOMAINS_MAX}")
        if facets:
            fdoms = tuple(dict.fromkeys(
                d.strip().lower() for d in facet_domains or ()
                if d and d.strip()))
            if len(fdoms) > FACET_MAX_DOMS:
                raise ValueError(
                    f"{len(fdoms)} facet domains; the cap is "
                    f"{FACET_MAX_DOMS} per query")
        # None leaves a plain request's key as it always was, and one
        # without top domains the key a facet request always had
        key = QueryCache.make_key(query, limit=limit, mode=mode,
                                  facets=None if fdoms is None
                                  else list(fdoms),
                                  top_domains=top or None,
                                  per_domain=cap or None)
        if use_cache:
            cached = self.cache.get(key)
            if cached is not None:
                return cached
        if deduct and self.config.credits.enabled:
            self.ledger.deduct_search_cost_async()
        self.related.record(query)
        authority = self.link_graph.url_authority
        trust_fn = self.trust.trust_fn()
        engine_ready = (self.engine is not None
                        and self.engine.shard.n_docs > 0)
        # Metadata filters (site:/language/date): by default filtered
        # queries take the FTS path even when the engine is up
        # (reference local_store.py:253-352 filter SQL); gpu.filters
        # sends them to the engine's masked top-k instead.
        pq = parse_query_filters(query)
        has_filters = bool(pq.site or pq.after or pq.before or pq.language
                           or pq.sites or pq.exclude_sites)
        if self.config.gpu.filters:
            has_filters = False
            if engine_ready and mode != "local":
                # over the cap: fail this caller here, not the whole
                # batch inside the batcher's executor
                pack_pred_sets(DocFilter(sites=pq.sites,
                                         exclude_sites=pq.exclude_sites))
        term_operators = self.config.gpu.term_operators
        if mode == "local" or (mode == "auto" and not engine_ready):
            resp = search_local(self.store, query, limit=limit,
                                authority_fn=authority, trust_fn=trust_fn,
                                boost_fn=(self.feedback.url_boost
                                          if self.feedback else None),
                                term_operators=term_operators)
        elif mode in ("auto", "hybrid", "distributed"):
            if engine_ready and not has_filters:
                # single-fusion path: the GPU plane RRF-fuses BM25 +
                # dense exactly once; results are hydrated from the
                # LocalStore (round-1 double-fusion fix)
                resp = self._engine_search(query, limit, mode,
                                           facet_domains=fdoms,
                                           top_domains=top, per_domain=cap)
                cap = 0
            else:
                resp = search_hybrid(
                    self.store, None, query, limit=limit,
                    authority_fn=authority, trust_fn=trust_fn,
                    rrf_k=self.config.search.rrf_k,
                    boost_fn=(self.feedback.url_boost
                              if self.feedback else None),
                    term_operators=term_operators)
                if mode == "distributed":
                    resp.mode = "distributed"
        else:
            raise InfoMeshError("SRCH001", f"unknown mode {mode!r}")
        if cap:
            # FTS served it: the cap can only thin out the hits it got
            # (quality.diversify's greedy pass, without the tail it
            # keeps: hits over the cap are dropped, not moved back)
            seen: Counter = Counter()
            kept = []
            for r in resp.results:
                seen[r.domain] += 1
                if seen[r.domain] <= cap:
                    kept.append(r)
            resp.results = kept
        if fdoms is not None and resp.facets is None:
            # FTS served it: SQLite hands back a LIMITed list, so the
            # counts can only cover the hits
            over = compute_facets(resp.results)
            resp.facets = {"scope": "results", "domains": over["domains"],
                           "languages": over["languages"],
                           "date_ranges": over["dates"]}
            if top:
                resp.facets["top_domains"] = dict(
                    Counter(r.domain for r in resp.results
                            if r.domain).most_common(top))
        resp = GLOBAL_PLUGINS.run("post_search", resp, query=query)
        if use_cache:
            self.cache.put(key, resp)
        self.ledger.record_action_async(Action.QUERY_SERVED, 1.0)
        return resp

    def ensure_batcher(self) -> QueryBatcher | None:
        """Create the micro-batcher if an engine was attached after
        create() (tests/benches assign ctx.engine directly)."""
        if self.batcher is None and self.engine is not None:
            self.batcher = QueryBatcher(
                self.engine, max_batch=self.config.search.batch_max,
                max_wait_ms=self.config.search.batch_wait_ms,
                execute=self._batch_execute)
        return self.batcher

    def make_auditor(self, fetch_fn):
        """Build the random-audit scheduler with the configured rate
        (trust.audits_per_hour) and quorum size (trust.auditors).
        fetch_fn: async url -> text | None (the node's own fetcher)."""
        from .trust.audit import AuditScheduler
        from .trust.detector import MaliciousNodeDetector
        return AuditScheduler(
            self.store, self.trust, fetch_fn,
            rate_per_hour=self.config.trust.audits_per_hour,
            auditors=self.config.trust.auditors,
            detector=MaliciousNodeDetector())

    def _batch_execute(self, queries: list[str],
                       limit: int) -> list[list]:
        """Batcher executor: ONE plane call + ONE hydration round trip
        for the whole batch (engine hits carry only global doc ids +
        fused scores; url/title/domain/snippet come from LocalStore).

        The GPU plane compares 32-bit domain hashes, so a hydrated hit
        is checked against the query's domain filters by name and
        dropped when its stored domain contradicts them. For site: that
        is a curiosity; for a 2048-entry list against ~1M distinct
        domains it is an expected event (2048 * 1M / 2^32 ~ 0.5 false
        matches per query), so the guard covers the lists too.

        With gpu.term_operators the +word / -word operators are split
        off the text here as well and go to the engine as require /
        exclude words. Term ids are buckets of a 2^17-entry hash, so a
        hit that passed a required word is re-checked against the
        stored text."""
        if self.batcher is not None \
                and self.batcher.engine is not self.engine:
            self.batcher.engine = self.engine   # engine was rebound
        # a facet request travels as a token in the text too
        # (nlp.with_facet_token): strip it, and build ONE spec for the
        # batch, one `now`, the fixed language list, and a domain list
        # per asking row. Rows that did not ask are not counted and get
        # the plain list they always got. An error here would fail every
        # caller of the batch, so a list over the cap (AppContext.search
        # refuses one on the caller's thread; only a direct submit can
        # bring one) is cut to its first FACET_MAX_DOMS names, never
        # raised.
        # A top-domain count over the cap is clamped likewise.
        asked, tops = [], []
        for text, doms, top in map(parse_facet_request, queries):
            asked.append((text,
                          doms if doms is None else doms[:FACET_MAX_DOMS]))
            tops.append(min(top, TOP_DOMAINS_MAX) if doms is not None else 0)
        # the per-site cap is a token as well (nlp.with_persite_token);
        # one out of range is clamped here, never raised
        capped = [parse_persite_token(text, clamp=True) for text, _ in asked]
        queries = [text for text, _ in capped]
        caps = [m for _, m in capped]
        spec = None
        if any(doms is not None for _, doms in asked):
            now = math.floor(time.time())
            spec = FacetSpec(
                date_edges=tuple(now - d * 86400 for d in _DATE_AGES_D)
                + (now + 1,),
                languages=known_languages(),
                domains=tuple(doms for _, doms in asked),
                top_domains=tuple(tops) if any(tops) else ())
        filters = None
        parsed: list = [None] * len(queries)
        if self.config.gpu.filters:
            # filter tokens travel inside the query text (the batcher's
            # signature knows nothing of them): split them off here,
            # score the stripped text, filter inside the plane's top-k
            parsed = [parse_query_filters(q) for q in queries]
            filters = [
                DocFilter(language=pq.language, site=pq.site,
                          after=pq.after, before=pq.before,
                          sites=pq.sites, exclude_sites=pq.exclude_sites)
                if (pq.site or pq.language or pq.after or pq.before
                    or pq.sites or pq.exclude_sites)
                else None for pq in parsed]
            queries = [pq.text for pq in parsed]
        required: list = [None] * len(queries)
        if self.config.gpu.term_operators:
            # +word / -word travel in the text as well: a required word
            # stays in it, an excluded one leaves it
            split = [parse_term_operators(q) for q in queries]
            queries = [text for text, _, _ in split]
            required = [
                {int(i) for w in req
                 for i in bm25_term_ids(w, vocab=_GUARD_VOCAB)} or None
                for _, req, _ in split]
            kw = dict(require=[req for _, req, _ in split],
                      exclude=[exc for _, _, exc in split])
        else:
            kw = {}
        if any(caps):
            kw["per_domain"] = caps
        counts: list = [None] * len(queries)
        if spec is None:
            per_q = self.engine.search_many(queries, limit=limit,
                                            filters=filters, **kw)
        else:
            per_q, counts = self.engine.search_with_facets(
                queries, limit=limit, filters=filters, facets=spec, **kw)
        gids = [h.doc_id for hits in per_q for h in hits]
        docs = self.store.get_documents(gids)
        out: list[list] = []
        for q, hits, pq, req in zip(queries, per_q, parsed, required):
            hydrated = []
            if self.config.gpu.term_operators and not q.strip():
                hits = []    # only exclusions: nothing to rank, as on FTS
            for h in hits:
                doc = docs.get(h.doc_id)
                if doc is None:
                    continue
                if pq is not None and (
                        (pq.site and doc.domain != pq.site)
                        or (pq.sites and doc.domain not in pq.sites)
                        or doc.domain in pq.exclude_sites):
                    continue   # 32-bit domain-hash collision guard
                if req is not None and doc.text and not req <= set(
                        bm25_term_ids(f"{doc.title}\n{doc.text}"[:4000],
                                      vocab=_GUARD_VOCAB).tolist()):
                    # (the text as HybridEngine.add_document cuts it)
                    # 2^17-bucket term-hash collision guard: the shard
                    # passed a document that holds only a word colliding
                    # with a required one. (An excluded word can only
                    # over-exclude, which no guard here can undo.)
                    continue
                h.url, h.title = doc.url, doc.title
                h.domain, h.crawled_at = doc.domain, doc.crawled_at
                if doc.text:
                    h.snippet = fast_snippet(q, doc.text)
                hydrated.append(h)
            if self.feedback is not None and hydrated \
                    and self.feedback.has_signals():
                # implicit-feedback boost on the GPU plane too: additive
                # on the fused RRF score, then reorder (cheap: <=limit
                # hits; url_boost is 60 s-cached per url)
                for h in hydrated:
                    h.score += self.feedback.url_boost(h.url)
                hydrated.sort(key=lambda x: x.score, reverse=True)
            out.append(hydrated)
        return [hits if doms is None else FacetedHits(hits, c)
                for hits, c, (_, doms) in zip(out, counts, asked)]

    @staticmethod
    def _facets_dict(c: FacetCounts) -> dict:
        """FacetCounts of the serving spec (_batch_execute) -> the
        "facets" dict of a SearchResponse."""
        ranges = dict(zip(_DATE_LABELS, c.dates))
        ranges["unknown"] += c.date_zero
        langs = dict(c.languages)
        langs["unknown"] = c.language_zero
        langs["other"] = c.language_other
        return {"scope": "matches", "domains": dict(c.domains),
                "languages": langs, "date_ranges": ranges}

    def _domain_label(self, h: int) -> str:
        """The name of a top domain's hash: the engine's map; on a miss
        (an engine started from a manifest never saw the names) the map
        is refilled once from the store's domains; "#%08x" for a hash
        that is still unknown."""
        name = self.engine.domain_name(h)
        if name is None and not self._domain_names_loaded:
            self._domain_names_loaded = True
            for d in self.store.all_domains():
                self.engine.note_domain(d)
            name = self.engine.domain_name(h)
        return name if name is not None else "#%08x" % h

    def _engine_search(self, query: str, limit: int, mode: str,
                       facet_domains=None,
                       top_domains: int = 0,
                       per_domain: int = 0) -> SearchResponse:
        """GPU-plane search via the micro-batcher (fused once on the
        plane, hydrated batch-wide in _batch_execute). facet_domains:
        None, or the domains to count of a request with facets;
        top_domains: how many top domains such a request asks for;
        per_domain: the per-site cap, 0 for none."""
        t0 = time.time()
        trace = None
        if self.otlp is not None and self.otlp.enabled:
            from .utils.observability import QueryTrace
            trace = QueryTrace(query)
        term_operators = self.config.gpu.term_operators
        # +word / -word tokens pass through verbatim, behind the text
        eff = preprocess_query(query, term_operators=term_operators)
        if term_operators:
            # over the operand cap: fail this caller here, not the whole
            # batch inside the batcher's executor; on the text as
            # _batch_execute will see it. Only the engine has a cap.
            text = eff
            if self.config.gpu.filters:
                text = parse_query_filters(text).text
            self.engine.term_ops_for(*parse_term_operators(text))
        # The one place that writes the facet token, from the capped
        # `facet_domains` alone and behind the preprocessed text, so
        # that effective_query stays without it. Preprocessing passes a
        # token through untouched, which is why AppContext.search drops
        # a typed one first; one that still came this way goes here.
        eff = parse_facet_token(eff)[0]
        # likewise the per-site token: written here alone
        eff = parse_persite_token(eff, clamp=True)[0]
        sent = with_persite_token(eff, per_domain)
        sent = sent if facet_domains is None \
            else with_facet_request(sent, facet_domains, top_domains)
        batcher = self.ensure_batcher()
        if trace is not None:
            with trace.span("engine"):
                hits = (batcher.submit(sent, limit) if batcher is not None
                        else self._batch_execute([sent], limit)[0])
            self.otlp.export(trace)
        elif batcher is not None:
            hits = batcher.submit(sent, limit)
        else:
            hits = self._batch_execute([sent], limit)[0]
        counts = None
        if isinstance(hits, FacetedHits):
            hits, counts = hits.hits[:limit], hits.counts
        resp = SearchResponse(
            query=query, effective_query=eff, results=hits,
            elapsed_ms=(time.time() - t0) * 1e3,
            mode="distributed" if mode == "distributed" else "hybrid",
            total_candidates=len(hits),
            degraded=bool(getattr(self.engine.plane.fabric,
                                  "degraded", False)))
        if facet_domains is not None and counts is not None:
            resp.total_matches = counts.total
            resp.facets = self._facets_dict(counts)
            if counts.top_domains is not None:
                resp.facets["top_domains"] = {
                    self._domain_label(h): n for h, n in counts.top_domains}
                resp.facets["top_domains_exact"] = counts.top_domains_exact
                resp.facets["top_domains_bound"] = counts.top_domains_bound
        return resp

    def fetch_page(self, url: str) -> Document | None:
        """Cache-first page fetch (reference: services.py:220-335);
        network fetch is the async crawl path."""
        return self.store.get_document_by_url(url)

    def flush_engine(self) -> int:
        if self.engine is None:
            return 0
        return self.engine.flush()

    # ------------------------------------------------------------- stats
    def status(self) -> dict[str, Any]:
        return {
            "node_id": self.keys.node_id,
            "role": self.config.node.role,
            "uptime_s": round(time.time() - self.started_at, 1),
            "index": self.store.stats(),
            "engine": self.engine.stats() if self.engine else None,
            "credits": self.ledger.stats(),
            "cache": self.cache.stats(),
            "batcher": self.batcher.stats() if self.batcher else None,
            "crawler": self.worker.stats if self.worker else None,
            "link_edges": self.link_graph.edge_count(),
        }

    def close(self) -> None:
        try:
            self.feeds.save()
        except Exception:
            pass
        if self.batcher is not None:
            self.batcher.close()
        for c in (self.store, self.link_graph, self.dedup, self.ledger,
                  self.trust, self.takedowns, self.deletions,
                  self.feedback):
            try:
                c.close()
            except Exception:
                pass


