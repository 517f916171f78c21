"""Query NLP: stop words, synonym expansion, did-you-mean, filter parsing.

Reference parity: infomesh/search/nlp.py (stop words for 9 languages,
synonym query expansion, edit-distance did-you-mean, natural-language
filter parsing site:/lang:/dates → ParsedQuery, related-search tracker).
"""
from __future__ import annotations

import math
import re
import time
from collections import OrderedDict
from dataclasses import dataclass, field

STOP_WORDS: dict[str, frozenset[str]] = {
    "en": frozenset("""a an and are as at be by for from has have he her his i in is it its
        of on or she that the their them they this to was we were what when where which who
        will with you your not no but if then so do does did can could should would about
        into over under after before between during above below again there here all any
        both each few more most other some such only own same than too very just""".split()),
    "de": frozenset("""der die das ein eine und oder aber nicht ist sind war waren ich du er
        sie es wir ihr mit von zu auf für in im am an als auch des dem den einer einem""".split()),
    "fr": frozenset("""le la les un une des et ou mais ne pas est sont était je tu il elle
        nous vous ils elles avec de du au aux pour dans sur par ce cette ces que qui""".split()),
    "es": frozenset("""el la los las un una unos unas y o pero no es son era yo tú él ella
        nosotros con de del al para en sobre por este esta estos estas que quien""".split()),
    "it": frozenset("""il lo la i gli le un uno una e o ma non è sono era io tu lui lei noi
        con di del al per in su da questo questa che chi""".split()),
    "pt": frozenset("""o a os as um uma uns umas e ou mas não é são era eu tu ele ela nós
        com de do da ao para em sobre por este esta que quem""".split()),
    "nl": frozenset("""de het een en of maar niet is zijn was ik jij hij zij wij met van
        naar op voor in aan als ook dit dat die""".split()),
    "ru": frozenset("""и в не на я он она оно мы вы они что это как но или же бы от до из
        у за по с к о для при так то все её его их""".split()),
    "ja": frozenset("""の に は を た が で て と し れ さ ある いる も する から な こと
        として い や など なっ ない この ため その あっ よう また もの""".split()),
}

_SYNONYMS: dict[str, list[str]] = {
    "fast": ["quick", "rapid"], "quick": ["fast"],
    "error": ["exception", "failure", "bug"], "bug": ["error", "defect"],
    "install": ["setup", "installation"], "setup": ["install"],
    "delete": ["remove", "erase"], "remove": ["delete"],
    "doc": ["documentation", "docs"], "docs": ["documentation"],
    "tutorial": ["guide", "howto"], "guide": ["tutorial"],
    "api": ["interface", "endpoint"],
    "config": ["configuration", "settings"], "settings": ["configuration"],
    "auth": ["authentication", "login"], "login": ["signin", "auth"],
    "example": ["sample", "demo"], "sample": ["example"],
    "performance": ["speed", "throughput"], "speed": ["performance"],
    "gpu": ["accelerator"], "ml": ["machine learning"],
    "db": ["database"], "database": ["db"],
    "async": ["asynchronous"], "sync": ["synchronous"],
}


def remove_stop_words(query: str, language: str = "en") -> str:
    sw = STOP_WORDS.get(language, STOP_WORDS["en"])
    kept = [t for t in query.split() if t.lower() not in sw]
    # Never empty the query entirely.
    return " ".join(kept) if kept else query


def expand_query(query: str, max_extra: int = 3) -> list[str]:
    """Return alternative query strings via the synonym table
    (used on sparse results — reference: search/query.py:136-156)."""
    terms = query.lower().split()
    out: list[str] = []
    for i, t in enumerate(terms):
        for syn in _SYNONYMS.get(t, []):
            alt = terms.copy()
            alt[i] = syn
            out.append(" ".join(alt))
            if len(out) >= max_extra:
                return out
    return out


# ------------------------------------------------------------ did-you-mean

def edit_distance(a: str, b: str, cap: int = 3) -> int:
    """Bounded Levenshtein distance."""
    if abs(len(a) - len(b)) > cap:
        return cap + 1
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        best = i
        for j, cb in enumerate(b, 1):
            c = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb))
            cur.append(c)
            best = min(best, c)
        if best > cap:
            return cap + 1
        prev = cur
    return prev[-1]


def did_you_mean(query: str, vocabulary: set[str] | dict[str, int],
                 max_distance: int = 2) -> str | None:
    """Suggest a corrected query when terms are near-misses of indexed
    vocabulary (reference: nlp.py:803-910). `vocabulary` may map
    term→frequency for tie-breaking."""
    freq = vocabulary if isinstance(vocabulary, dict) else {t: 1 for t in vocabulary}
    corrected: list[str] = []
    changed = False
    for term in query.split():
        tl = term.lower()
        if tl in freq or len(tl) < 3:
            corrected.append(term)
            continue
        best, best_d, best_f = None, max_distance + 1, 0
        for cand, f in freq.items():
            d = edit_distance(tl, cand, cap=max_distance)
            if d < best_d or (d == best_d and f > best_f):
                if d <= max_distance:
                    best, best_d, best_f = cand, d, f
        if best is not None:
            corrected.append(best)
            changed = True
        else:
            corrected.append(term)
    return " ".join(corrected) if changed else None


# ------------------------------------------------------- filter parsing

@dataclass
class ParsedQuery:
    text: str
    site: str | None = None
    language: str | None = None
    after: float | None = None
    before: float | None = None
    raw: str = ""
    # domain lists, matched exactly on the stored domain: site:a.org,b.org
    # allows only these, -site:a.org[,b.org] blocks them
    sites: tuple[str, ...] = ()
    exclude_sites: tuple[str, ...] = ()


# a minus belongs to the filter only in front of site: at the start of a
# token; anywhere else it stays in the text as it always did
_FILTER_RE = re.compile(
    r"(?:(?<!\S)(-)(?=site:))?\b(site|lang|language|before|after):(\S+)",
    re.I)
_DATE_FMTS = ("%Y-%m-%d", "%Y/%m/%d", "%Y-%m", "%Y")


def _parse_date(text: str) -> float | None:
    if text.startswith("@"):          # @<epoch seconds>
        try:
            return float(text[1:])
        except ValueError:
            return None
    for fmt in _DATE_FMTS:
        try:
            return time.mktime(time.strptime(text, fmt))
        except ValueError:
            continue
    return None


def parse_query_filters(query: str) -> ParsedQuery:
    """Extract site:/lang:/before:/after: filters from the query text
    (reference: nlp.py:911-971). site: with two or more comma-separated
    names is an allow list and -site: a block list (with_filter_tokens
    writes both); dates also come as @<epoch seconds>."""
    pq = ParsedQuery(text=query, raw=query)
    def _sub(m: re.Match) -> str:
        minus, key, val = m.group(1), m.group(2).lower(), m.group(3)
        names = _site_names(val) if key == "site" else ()
        if minus:
            pq.exclude_sites += tuple(
                n for n in names if n not in pq.exclude_sites)
        elif key == "site" and "," in val:
            pq.sites += tuple(n for n in names if n not in pq.sites)
        elif key == "site":
            pq.site = val.lower().lstrip("www.") if val.startswith("www.") else val.lower()
        elif key in ("lang", "language"):
            pq.language = val.lower()[:2]
        elif key == "before":
            pq.before = _parse_date(val)
        elif key == "after":
            pq.after = _parse_date(val)
        return ""
    pq.text = _FILTER_RE.sub(_sub, query).strip()
    pq.text = re.sub(r"\s{2,}", " ", pq.text)
    return pq


# +word / -word: the sign counts only at the start of a token and
# directly before a word character; the token runs to the next white
# space. A token with a colon (-site:a.org, +lang:de) is filter syntax
# and is left alone.
_TERM_OP_RE = re.compile(r"(?<!\S)([+-])(\w[^\s:]*)(?!\S)")


def is_term_operator(token: str) -> bool:
    """Is this white-space-delimited token a +word / -word operator?"""
    return _TERM_OP_RE.fullmatch(token) is not None


def parse_term_operators(text: str
                         ) -> tuple[str, tuple[str, ...], tuple[str, ...]]:
    """Split the +word / -word operators off a query (applied to the
    text parse_query_filters leaves) -> (text, require_words,
    exclude_words). A required word stays in the text without its plus,
    so it is still scored; an excluded word leaves the text. A bare
    "-", a hyphen inside a word ("well-known") and "-site:" are not
    operators and stay as they are. Words come back lower-cased, without
    repeats, in order of appearance."""
    require: list[str] = []
    exclude: list[str] = []

    def _sub(m: re.Match) -> str:
        sign, word = m.group(1), m.group(2)
        (require if sign == "+" else exclude).append(word.lower())
        return word if sign == "+" else ""
    out = _TERM_OP_RE.sub(_sub, text)
    if not require and not exclude:
        return text, (), ()
    out = re.sub(r"\s{2,}", " ", out).strip()
    return (out, tuple(dict.fromkeys(require)),
            tuple(dict.fromkeys(exclude)))


def _site_names(val: str) -> tuple[str, ...]:
    """The lower-cased names of a comma-separated site value, in order,
    without repeats. Lists match the stored domain exactly, so a
    leading www. stays."""
    return tuple(dict.fromkeys(
        n for n in (p.strip().lower() for p in val.split(",")) if n))


def with_filter_tokens(query: str, include=(), exclude=(),
                       after: float | None = None) -> str:
    """`query` with the tokens appended that parse_query_filters reads
    back as (sites, exclude_sites, after): the one writer of that
    syntax. A one-name allow list is written with the name twice, since
    one name alone is the site: form; white space and commas, which no
    host name holds, turn into '_' so that such a name keeps its place
    in the list and matches nothing."""
    def names(domains) -> list[str]:
        return list(_site_names(",".join(
            re.sub(r"[\s,]+", "_", d.strip()) for d in domains or ()
            if d and d.strip())))
    inc, exc = names(include), names(exclude)
    parts = [query]
    if inc:
        parts.append("site:" + ",".join(inc * 2 if len(inc) == 1 else inc))
    if exc:
        parts.append("-site:" + ",".join(exc))
    if after is not None:
        parts.append(f"after:@{int(math.ceil(after))}")
    return " ".join(parts)


# A facet request travels to the engine as one token at the end of the
# query text, like the filters do: facets:@ and the domains to count,
# comma-separated (facets:@ alone: no domain counts). A request for the
# match set's top T domains writes T between the colon and the @:
# facets:20@a.com,b.com. No other code reads or writes this syntax.
_FACET_RE = re.compile(r"(?<!\S)facets:(\d*)@(\S*)(?!\S)")


def _facet_names(domains) -> tuple[str, ...]:
    """Names as with_filter_tokens writes a list's."""
    return _site_names(",".join(
        re.sub(r"[\s,]+", "_", d.strip()) for d in domains or ()
        if d and d.strip()))


def with_facet_token(query: str, domains=()) -> str:
    """`query` with the token appended that parse_facet_token reads
    back: the one writer of that syntax for a request without top
    domains (with_facet_request writes the others)."""
    return f"{query} facets:@{','.join(_facet_names(domains))}".lstrip()


def with_facet_request(query: str, domains=(), top: int = 0) -> str:
    """with_facet_token for a request that may ask for its top `top`
    domains as well; top = 0 writes with_facet_token's token."""
    if not top:
        return with_facet_token(query, domains)
    return f"{query} facets:{int(top)}@" \
           f"{','.join(_facet_names(domains))}".lstrip()


def parse_facet_request(query: str
                        ) -> tuple[str, tuple[str, ...] | None, int]:
    """(text without the token, domains to count, top domains asked for)
    of a query with_facet_token or with_facet_request wrote;
    (query, None, 0) when it carries no token. The number is whatever
    was written: the reader clamps it."""
    found: list[tuple[tuple[str, ...], int]] = []

    def _sub(m: re.Match) -> str:
        found.append((_site_names(m.group(2)), int(m.group(1) or 0)))
        return ""
    text = _FACET_RE.sub(_sub, query)
    if not found:
        return query, None, 0
    return re.sub(r"\s{2,}", " ", text).strip(), *found[-1]


def parse_facet_token(query: str) -> tuple[str, tuple[str, ...] | None]:
    """(text without the token, domains to count) of a query
    with_facet_token wrote; (query, None) when it carries no token."""
    return parse_facet_request(query)[:2]


# A per-domain cap travels as one token of the query text, like the
# filters do: persite:N, at most N hits per site, 1 <= N <= PERSITE_MAX
# (the GPU plane's COLLAPSE_M_MAX). No other code reads or writes this
# syntax.
PERSITE_MAX = 4
_PERSITE_RE = re.compile(r"(?<!\S)persite:(\d+)(?!\S)")


def with_persite_token(query: str, m: int = 0) -> str:
    """`query` with the token appended that parse_persite_token reads
    back; m = 0 (or None) appends nothing. m outside 0 .. PERSITE_MAX is
    a ValueError."""
    m = int(m or 0)
    if not 0 <= m <= PERSITE_MAX:
        raise ValueError(f"per_domain = {m}; 0 (no cap) or 1 .. {PERSITE_MAX}")
    return f"{query} persite:{m}".lstrip() if m else query


def parse_persite_token(query: str, clamp: bool = False
                        ) -> tuple[str, int]:
    """(text without the token, cap) of a query with a persite:N token;
    (query, 0) when it carries none; the last one counts. N outside
    1 .. PERSITE_MAX is a ValueError, so that a typed token fails its
    caller; clamp=True (the batch executor, where an error would fail
    every caller of the batch) brings N into the range instead."""
    found: list[int] = []

    def _sub(m: re.Match) -> str:
        found.append(int(m.group(1)))
        return ""
    text = _PERSITE_RE.sub(_sub, query)
    if not found:
        return query, 0
    n = found[-1]
    if not 1 <= n <= PERSITE_MAX:
        if not clamp:
            raise ValueError(f"persite:{n}; 1 <= N <= {PERSITE_MAX}")
        n = min(max(n, 1), PERSITE_MAX)
    return re.sub(r"\s{2,}", " ", text).strip(), n


# ---------------------------------------------------- related searches

@dataclass
class RelatedSearchTracker:
    """Session-local co-occurrence tracker for `related searches`
    (reference: nlp.py:972+). Locked: the MCP HTTP transport records
    from many handler threads, and an unguarded OrderedDict iteration
    concurrent with a record() raises mid-request."""
    max_entries: int = 1000
    _recent: OrderedDict = field(default_factory=OrderedDict)
    _lock: "threading.Lock" = field(
        default_factory=lambda: __import__("threading").Lock())

    def record(self, query: str) -> None:
        q = query.strip().lower()
        if not q:
            return
        with self._lock:
            self._recent[q] = self._recent.pop(q, 0) + 1
            while len(self._recent) > self.max_entries:
                self._recent.popitem(last=False)

    def related(self, query: str, limit: int = 5) -> list[str]:
        terms = set(query.lower().split())
        if not terms:
            return []
        with self._lock:
            snapshot = list(self._recent.items())
        scored = []
        for past, cnt in snapshot:
            if past == query.lower():
                continue
            overlap = len(terms & set(past.split()))
            if overlap:
                scored.append((overlap * cnt, past))
        scored.sort(reverse=True)
        return [p for _, p in scored[:limit]]


def extract_keywords(text: str, top_n: int = 50, min_len: int = 2,
                     language: str = "en") -> list[tuple[str, int]]:
    """TF-based keyword extraction (reference: index/distributed.py:
    30-159, where it fed the DHT keyword->pointer publish; here the GPU
    shard indexes every term exhaustively, so this serves faceting,
    related-search seeding and summary key-fact hints).

    Returns (keyword, count) pairs, most frequent first, stop-worded
    and length-filtered, capped at top_n."""
    from collections import Counter
    sw = STOP_WORDS.get(language, STOP_WORDS["en"])
    words = re.findall(r"[\w'-]+", text.lower())
    counts = Counter(w for w in words
                     if len(w) >= min_len and w not in sw
                     and not w.isdigit())
    return counts.most_common(top_n)
