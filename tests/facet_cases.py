"""What the facet tests share (CPU and GPU): the FacetSpec they put on
tests/term_ops_corpus.py's batch, and the brute-force count of one row
from the corpus' own ground truth."""
from __future__ import annotations

import term_ops_corpus as C
from infomesh_amd.index.doc_attrs import FacetCounts, FacetSpec

FACET_DOMAINS = tuple(C.DOMAINS) + ("absent.example",)
# on the first document of segments two and three, and past every document
EDGES = (C.T0 + 45, C.T0 + 345, C.T0 + 10_000)


def corpus_spec(n_rows: int) -> FacetSpec:
    """Facets on every row; the rows' domain lists differ in width."""
    return FacetSpec(date_edges=EDGES, languages=("de", "en", "xx"),
                     domains=tuple(FACET_DOMAINS[i % 3:]
                                   for i in range(n_rows)))


def brute_counts(terms, filters, ops, meta, sets, spec, qi) -> FacetCounts:
    """Row qi, document by document: C.passes(...) and a query term in
    the document's token set."""
    edges = sorted(set(spec.date_edges))
    total, dates = 0, [0] * (len(edges) + 1)
    langs = {c: 0 for c in spec.languages}
    other = 0
    dom = {d: 0 for d in spec.domains[qi]}
    for i in range(C.N_DOCS):
        if not (C.passes(C.GID0 + i, meta, filters[qi], ops[qi], sets)
                and set(terms[qi].tolist()) & sets[i]):
            continue
        lang, d, crawled = meta[i]
        total += 1
        dates[sum(1 for e in edges if e <= crawled)] += 1
        if lang in langs:
            langs[lang] += 1
        else:
            other += 1
        if d in dom:
            dom[d] += 1
    return FacetCounts(total=total, date_zero=0, dates=tuple(dates),
                       languages=langs, language_zero=0, language_other=other,
                       domains=dom)
