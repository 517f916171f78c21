"""Per-document filter attributes and query predicates, as packed words.

The one Python packer for the 16-byte attribute record and the 16-byte
predicate that the GPU filter kernel reads; the layout itself is written
down once, in the header of ops/csrc/docfilter.hip. Replaces on the GPU
plane: the reference's SQL filters on the documents table
(infomesh/index/local_store.py, language/domain/crawled_at columns).

Words are unsigned 32-bit values; tensors carry them as int32 with the
same bits (torch has no uint32 arithmetic worth relying on).
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from ..hashing import hash64

LANG_MASK = 0xFFFF
DEAD_BIT = 1 << 16      # attribute word 1
HAS_SITE_BIT = 1 << 16  # predicate word z
# bit 17 of z is the query plane's in-transit "row has a filter" mark
HAS_ALLOW_BIT = 1 << 18  # predicate word z: an allow list goes with it
HAS_BLOCK_BIT = 1 << 19  # predicate word z: a block list goes with it
MAX_LIST_HASHES = 2048   # per predicate, allow and block together
U32_MAX = 0xFFFFFFFF


def lang16(language: str | None) -> int:
    """ord(c0)<<8 | ord(c1) of the lower-cased 2-letter code; 0 for
    unknown (None, empty, or not two ASCII characters)."""
    code = (language or "").strip().lower()[:2]
    if len(code) != 2 or not code.isascii():
        return 0
    return (ord(code[0]) << 8) | ord(code[1])


def domain_hash(domain: str | None) -> int:
    """Low 32 bits of hash64 of the lower-cased domain, as
    `extract_domain` / LocalStore store it."""
    return hash64((domain or "").strip().lower()) & U32_MAX


def _clamp_u32(v: float) -> int:
    return int(min(max(v, 0), U32_MAX))


def pack_attrs(language: str | None, domain: str | None,
               crawled_at: float | None) -> tuple[int, int, int, int]:
    """One document's attribute words (w0, w1, w2, w3). `crawled_at` is
    truncated to whole seconds. The dead bit is never set here; only
    `GpuShard.delete` sets it."""
    return (_clamp_u32(math.floor(crawled_at or 0.0)), lang16(language),
            domain_hash(domain), 0)


@dataclass(frozen=True)
class DocFilter:
    """A query's metadata restriction; every None field is unrestricted.

    Date bounds compare WHOLE seconds on the GPU plane: `after` is
    rounded up and `before` is rounded down, then a document passes iff
    after <= floor(crawled_at) <= before. SQLite compares the REAL
    column, so the two planes can differ for a document crawled within
    the same second as a fractional bound."""
    language: str | None = None
    site: str | None = None
    after: float | None = None
    before: float | None = None
    # domain lists, matched exactly on the stored (lower-cased) domain:
    # with `sites` a document's domain must be one of them, and it must
    # never be one of `exclude_sites` (a domain in both is blocked);
    # `site` and `sites` together must both hold
    sites: tuple[str, ...] = ()
    exclude_sites: tuple[str, ...] = ()


TERM_OPS_MAX = 16   # operands per query row, require and exclude together


@dataclass(frozen=True)
class TermOps:
    """A query row's required and excluded terms (+word / -word), as
    hashed BM25 term ids (gpu_index.bm25_term_ids). A document passes
    iff it holds EVERY require id and NO exclude id; both planes select
    among the passing documents only (layout and kernel:
    ops/csrc/termmask.hip).

    A require id that occurs nowhere in the shard fails every document
    (the row pads with -inf / -1), and an id in both lists passes
    nothing. Build one with TermOps.of, which dedupes; more than
    TERM_OPS_MAX operands in the two lists together is a ValueError."""
    require: tuple[int, ...] = ()
    exclude: tuple[int, ...] = ()

    def __post_init__(self):
        n = len(self.require) + len(self.exclude)
        if n > TERM_OPS_MAX:
            raise ValueError(
                f"{n} term operands; the cap is {TERM_OPS_MAX} per query, "
                f"required and excluded together")
        if any(t < 0 for t in self.require + self.exclude):
            raise ValueError("term ids are non-negative")

    @classmethod
    def of(cls, require=(), exclude=()) -> "TermOps":
        """From any iterables of ids: each list deduped, order kept."""
        return cls(tuple(dict.fromkeys(int(t) for t in require)),
                   tuple(dict.fromkeys(int(t) for t in exclude)))

    def __bool__(self) -> bool:
        return bool(self.require or self.exclude)


FACET_MAX_EDGES = 7     # date edges per batch      (ops/csrc/facets.hip)
FACET_MAX_LANGS = 32    # listed languages per batch
FACET_MAX_DOMS = 64     # domain hashes per row
TOP_DOMAINS_MAX = 32    # top domains a row may ask for (T)
# What every shard reports per top row: its first TOP_FETCH domains, and
# one more entry whose count is the shard's cut-off (ops/csrc/domtop.hip
# selects TOP_FETCH + 1; the query plane merges the reports).
TOP_FETCH = 64


def facet_slots(E: int, L: int) -> dict[str, int]:
    """First slot of every group of a facet count row for E date edges
    and L listed languages; the layout is written down in the header of
    ops/csrc/facets.hip, and the extension reports the same numbers
    (ops/kernels.facet_slots)."""
    return {"total": 0, "date_zero": 1, "date0": 2, "lang_zero": 3 + E,
            "lang0": 4 + E, "lang_other": 4 + E + L, "dom0": 5 + E + L}


def facet_width(E: int, L: int, Dw: int) -> int:
    """Slots per count row: Dw is the widest domain list of the batch."""
    return 5 + E + L + Dw


@dataclass(frozen=True)
class FacetSpec:
    """What to count over a batch's match sets. A document matches a
    row iff it passes the row's filter, domain lists and term operands,
    is not deleted, and holds at least one of the row's query terms
    (BM25 score > 0); the dense plane takes no part.

    date_edges: u32 seconds, one list per batch; a document with
    crawled_at != 0 falls into bucket #{edges <= floor(crawled_at)}.
    languages: 2-letter codes, one list per batch. domains: one entry
    per row, a tuple of domain names to count or None for a row that is
    not counted. Domains count by their 32-bit hash (domain_hash), as
    the filters compare them: two names with one hash share a count.

    top_domains: one T per row, 0 (or a missing entry) for none: the
    first T domains of the row's whole match set by count descending,
    then hash ascending as unsigned, whatever the caller listed. T is
    at most TOP_DOMAINS_MAX, and a row with T > 0 is a counted row
    (domains[i] is not None; () will do)."""
    date_edges: tuple[int, ...] = ()
    languages: tuple[str, ...] = ()
    domains: tuple[tuple[str, ...] | None, ...] = ()
    top_domains: tuple[int, ...] = ()


@dataclass(frozen=True)
class FacetCounts:
    """One row's counts, mapped back to the caller's FacetSpec.
    dates[i]: documents with exactly i of the sorted, deduped edges
    <= crawled_at (len(edges) + 1 buckets); date_zero: crawled_at == 0.
    languages / domains: one count per name, in the caller's order.
    total == date_zero + sum(dates) == language_zero + language_other
    + (the counts of the distinct listed languages).

    top_domains: None unless the row asked for top domains, else its
    (hash, count) pairs in order; every count is exact over all serving
    shards. top_domains_exact: the pairs are the true first T. When it
    is False a domain that is not shown may hold up to
    top_domains_bound matches (the sum of the shards' cut-offs) and
    belong among them."""
    total: int
    date_zero: int
    dates: tuple[int, ...]
    languages: dict
    language_zero: int
    language_other: int
    domains: dict
    top_domains: tuple[tuple[int, int], ...] | None = None
    top_domains_exact: bool = True
    top_domains_bound: int = 0


@dataclass(frozen=True)
class PackedFacets:
    """A FacetSpec as the kernel reads it (and as the query plane
    forwards it between ranks): edges and language codes ascending and
    unique, `rows` the counted batch rows, `lists` each one's domain
    hashes, unique and ascending as unsigned. top: one T per counted
    row (0: no top domains), or () when no row asked."""
    edges: tuple[int, ...]
    langs: tuple[int, ...]
    rows: tuple[int, ...]
    lists: tuple[tuple[int, ...], ...]
    top: tuple[int, ...] = ()

    def __post_init__(self):
        if any(t < 0 or t > TOP_DOMAINS_MAX for t in self.top):
            raise ValueError(
                f"facets: top domains {max(self.top)} / {min(self.top)}; "
                f"0 <= T <= {TOP_DOMAINS_MAX}")
        assert len(self.top) in (0, len(self.rows))
        widest = max((len(h) for h in self.lists), default=0)
        if len(self.edges) > FACET_MAX_EDGES \
                or len(self.langs) > FACET_MAX_LANGS \
                or widest > FACET_MAX_DOMS:
            raise ValueError(
                f"facets: {len(self.edges)} date edges, {len(self.langs)} "
                f"languages, {widest} domains in one row; the caps are "
                f"{FACET_MAX_EDGES}, {FACET_MAX_LANGS} and {FACET_MAX_DOMS}")
        assert len(self.rows) == len(self.lists)

    @property
    def width(self) -> int:
        return facet_width(len(self.edges), len(self.langs),
                           max((len(h) for h in self.lists), default=0))

    @property
    def top_rows(self) -> tuple[int, ...]:
        """The batch rows that asked for top domains, in `rows` order."""
        return tuple(b for b, t in zip(self.rows, self.top) if t > 0)

    def tables(self):
        """(rows [R], edges [E], langs [L], dom_desc [R, 2], doms) as
        int32 arrays with the u32 bits, for facet_counts."""
        def u32(v):
            return np.asarray(v, dtype=np.uint32).view(np.int32)
        desc = np.zeros((len(self.rows), 2), dtype=np.int32)
        flat: list[int] = []
        for r, h in enumerate(self.lists):
            desc[r] = (len(flat), len(h))
            flat.extend(h)
        return (np.asarray(self.rows, dtype=np.int32), u32(self.edges),
                u32(self.langs), desc, u32(flat))


def pack_facets(spec, B: int) -> PackedFacets | None:
    """FacetSpec -> PackedFacets for a batch of B rows (spec.domains may
    be shorter: the rows past its end are not counted); a PackedFacets
    passes through. None when no row is counted. Over a cap, or a
    language that is no 2-letter ASCII code, is a ValueError."""
    if spec is None or isinstance(spec, PackedFacets):
        return spec if spec is None or spec.rows else None
    if len(spec.domains) > B:
        raise ValueError("facets: more domain lists than rows")
    codes = [lang16(c) for c in spec.languages]
    if 0 in codes:
        raise ValueError("facets: languages are 2-letter ASCII codes")
    if len(spec.top_domains) > B:
        raise ValueError("facets: more top-domain entries than rows")
    tops = {i: int(t) for i, t in enumerate(spec.top_domains) if t}
    for i, t in tops.items():
        if t < 0 or t > TOP_DOMAINS_MAX:
            raise ValueError(
                f"facets: row {i} asks for {t} top domains; "
                f"0 <= T <= {TOP_DOMAINS_MAX}")
        if i >= len(spec.domains) or spec.domains[i] is None:
            raise ValueError(
                f"facets: row {i} asks for top domains but is not a "
                f"counted row (domains[{i}] is None)")
    rows = tuple(i for i, d in enumerate(spec.domains) if d is not None)
    if not rows:
        return None
    return PackedFacets(
        edges=tuple(sorted({_clamp_u32(e) for e in spec.date_edges})),
        langs=tuple(sorted(set(codes))), rows=rows,
        lists=tuple(_hash_list(spec.domains[i]) for i in rows),
        top=tuple(tops.get(i, 0) for i in rows) if tops else ())


def facet_results(spec: FacetSpec, packed: PackedFacets | None,
                  counts, n_rows: int | None = None, top=None
                  ) -> list[FacetCounts | None]:
    """counts [R, F] (the rows of `packed`, any integer array-like) ->
    one FacetCounts or None per batch row, in the caller's names and
    order: the permutation back from pack_facets' sorting. top: None, or
    one (pairs, exact, bound) per row of packed.top_rows, as the query
    plane merges them; each is cut to the row's T here."""
    tops = {}
    if packed is not None and top is not None:
        t_of = dict(zip(packed.rows, packed.top))
        for b, (pairs, exact, bound) in zip(packed.top_rows, top):
            tops[b] = dict(
                top_domains=tuple((int(h), int(c))
                                  for h, c in pairs[:t_of[b]]),
                top_domains_exact=bool(exact), top_domains_bound=int(bound))
    n = len(spec.domains) if n_rows is None else n_rows
    out: list[FacetCounts | None] = [None] * n
    if packed is None:
        return out
    c = np.asarray(counts).astype(np.int64).reshape(len(packed.rows), -1)
    E, L = len(packed.edges), len(packed.langs)
    sl = facet_slots(E, L)
    lang_at = {code: i for i, code in enumerate(packed.langs)}
    for r, (b, hashes) in enumerate(zip(packed.rows, packed.lists)):
        if b >= n:
            continue
        dom_at = {h: i for i, h in enumerate(hashes)}
        out[b] = FacetCounts(
            total=int(c[r, sl["total"]]),
            date_zero=int(c[r, sl["date_zero"]]),
            dates=tuple(int(v) for v in
                        c[r, sl["date0"]:sl["date0"] + E + 1]),
            languages={name: int(c[r, sl["lang0"] + lang_at[lang16(name)]])
                       for name in spec.languages},
            language_zero=int(c[r, sl["lang_zero"]]),
            language_other=int(c[r, sl["lang_other"]]),
            domains={name: int(c[r, sl["dom0"] + dom_at[domain_hash(name)]])
                     for name in spec.domains[b]},
            **tops.get(b, {}))
    return out


def domain_tables_np(attrs: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """(dom_keys [D], dom_id [N]) of attrs [N, 4], as int32: the distinct
    w2 words ascending as unsigned (their u32 bits), and every row's index
    into them. The tables a shard keeps per epoch for domain_count."""
    a = np.ascontiguousarray(attrs).view(np.uint32).reshape(-1, 4)
    keys, inv = np.unique(a[:, 2], return_inverse=True)
    return keys.view(np.int32), inv.reshape(-1).astype(np.int32)


def domain_top_np(scores: np.ndarray, fail: np.ndarray | None,
                  attrs: np.ndarray, rows, K: int) -> np.ndarray:
    """The oracle of top domains: scores [B, N], fail bool [B, N] or
    None, attrs [N, 4], rows the batch rows to count -> [R, K, 2] int32
    of (hash bits, count) pairs: per row the first K domains (w2 words)
    of the matching documents (FacetSpec's rule) by count descending,
    then hash ascending as unsigned; (0, 0) past the last one."""
    a = np.ascontiguousarray(attrs).view(np.uint32).reshape(-1, 4)
    out = np.zeros((len(rows), K, 2), dtype=np.int64)
    for r, b in enumerate(rows):
        m = scores[b] > 0
        if fail is not None:
            m = m & ~fail[b]
        keys, cnt = np.unique(a[m, 2], return_counts=True)
        order = np.lexsort((keys, -cnt.astype(np.int64)))[:K]
        out[r, :len(order), 0] = keys[order]
        out[r, :len(order), 1] = cnt[order]
    return out.astype(np.uint32).view(np.int32)


def facet_counts_np(scores: np.ndarray, fail: np.ndarray | None,
                    attrs: np.ndarray, packed: PackedFacets) -> np.ndarray:
    """The counts in numpy, for CpuShard: scores [B, N], fail bool
    [B, N] or None, attrs [N, 4] -> [R, F] int32, by the rules of
    FacetSpec and the layout of facet_slots."""
    a = np.ascontiguousarray(attrs).view(np.uint32).reshape(-1, 4)
    E, L = len(packed.edges), len(packed.langs)
    sl = facet_slots(E, L)
    edges = np.asarray(packed.edges, dtype=np.uint32)
    code = a[:, 1] & np.uint32(LANG_MASK)
    date = np.where(a[:, 0] == 0, sl["date_zero"],
                    sl["date0"] + np.searchsorted(edges, a[:, 0],
                                                  side="right"))
    lang = np.full(len(a), sl["lang_other"], dtype=np.int64)
    for i, c in enumerate(packed.langs):
        lang[code == np.uint32(c)] = sl["lang0"] + i
    lang[code == 0] = sl["lang_zero"]
    F = packed.width
    out = np.zeros((len(packed.rows), F), dtype=np.int64)
    for r, (b, hashes) in enumerate(zip(packed.rows, packed.lists)):
        m = scores[b] > 0
        if fail is not None:
            m &= ~fail[b]
        out[r, sl["total"]] = m.sum()
        out[r] += np.bincount(date[m], minlength=F)
        out[r] += np.bincount(lang[m], minlength=F)
        for i, h in enumerate(hashes):
            out[r, sl["dom0"] + i] = (m & (a[:, 2] == np.uint32(h))).sum()
    return out.astype(np.int32)


def _is_packed_sets(f) -> bool:
    """(words4, allow_hashes, block_hashes), the form pack_pred_sets
    returns and the query plane forwards between ranks."""
    return isinstance(f, tuple) and len(f) == 3 and isinstance(f[0], tuple)


def pack_pred(f) -> tuple[int, int, int, int]:
    """Predicate words (x, y, z, w) of a DocFilter; None is the
    live-only predicate. A 4-tuple is taken as words already packed
    (the query plane forwards predicates between ranks in that form).
    A filter with domain lists has no 4-word form: pack_pred_sets."""
    if f is None:
        return (0, U32_MAX, 0, 0)
    if isinstance(f, tuple) and not _is_packed_sets(f):
        x, y, z, w = (int(v) & U32_MAX for v in f)
        return (x, y, z, w)
    words, allow, block = pack_pred_sets(f)
    if allow or block:
        raise ValueError("filter carries domain lists: use pack_pred_sets")
    return words


def _hash_list(domains) -> tuple[int, ...]:
    """domain_hash of every name, unique, ascending as unsigned 32-bit."""
    return tuple(sorted({domain_hash(d) for d in domains}))


def pack_pred_sets(f) -> tuple[tuple[int, int, int, int],
                               tuple[int, ...], tuple[int, ...]]:
    """(words4, allow_hashes, block_hashes) of a filter with or without
    domain lists. The hashes are domain_hash values, unique and sorted
    ascending as unsigned 32-bit; bits 18 / 19 of word z say that the
    allow / block list is non-empty. Accepts what pack_pred accepts and
    its own result (which passes through). More than MAX_LIST_HASHES
    hashes in the two lists together is a ValueError."""
    if _is_packed_sets(f):
        words, allow, block = f
        allow = tuple(int(h) & U32_MAX for h in allow)
        block = tuple(int(h) & U32_MAX for h in block)
        words = pack_pred(words)
    elif f is None or isinstance(f, tuple):
        return pack_pred(f), (), ()
    else:
        allow, block = _hash_list(f.sites), _hash_list(f.exclude_sites)
        words = _pack_words(f)
    if len(allow) + len(block) > MAX_LIST_HASHES:
        raise ValueError(
            f"domain lists hold {len(allow) + len(block)} hashes; the cap "
            f"is {MAX_LIST_HASHES} per predicate, allow and block together")
    x, y, z, w = words
    z &= ~(HAS_ALLOW_BIT | HAS_BLOCK_BIT)
    if allow:
        z |= HAS_ALLOW_BIT
    if block:
        z |= HAS_BLOCK_BIT
    return (x, y, z, w), allow, block


def _pack_words(f: DocFilter) -> tuple[int, int, int, int]:
    """The four words of a DocFilter's non-list fields."""
    x = 0 if f.after is None else _clamp_u32(math.ceil(f.after))
    y = U32_MAX if f.before is None else _clamp_u32(math.floor(f.before))
    z = lang16(f.language)
    w = 0
    if f.site:
        z |= HAS_SITE_BIT
        w = domain_hash(f.site)
    return (x, y, z, w)


def words_i32(rows) -> np.ndarray:
    """[n, 4] u32 words -> the int32 array with the same bits."""
    return np.asarray(rows, dtype=np.uint32).reshape(-1, 4).view(np.int32)


def passes(attrs: np.ndarray, pred, allow=None, block=None) -> np.ndarray:
    """The predicate in numpy: attrs [N, 4] (int32 or uint32 bits), pred
    4 words -> bool [N]. CpuShard and the bitmask oracle both use it.
    allow / block: u32 domain hashes (any int dtype with those bits); a
    non-empty allow list must hold the document's w2, a block list must
    not. As in the kernel, the lists' lengths decide, not the flag bits."""
    a = np.ascontiguousarray(attrs).view(np.uint32).reshape(-1, 4)
    x, y, z, w = (int(v) & U32_MAX for v in pred)
    qlang = z & LANG_MASK
    ok = (a[:, 1] & np.uint32(DEAD_BIT)) == 0
    ok &= (a[:, 0] >= np.uint32(x)) & (a[:, 0] <= np.uint32(y))
    if qlang:
        ok &= (a[:, 1] & np.uint32(LANG_MASK)) == np.uint32(qlang)
    if z & HAS_SITE_BIT:
        ok &= a[:, 2] == np.uint32(w)
    if allow is not None and len(allow):
        ok &= np.isin(a[:, 2], _as_u32(allow))
    if block is not None and len(block):
        ok &= ~np.isin(a[:, 2], _as_u32(block))
    return ok


def _as_u32(hashes) -> np.ndarray:
    h = np.asarray(hashes)
    if h.dtype.itemsize == 4:
        return np.ascontiguousarray(h).view(np.uint32)
    return (h.astype(np.int64) & U32_MAX).astype(np.uint32)
