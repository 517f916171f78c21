"""The corpus the term-operand tests share (CPU and GPU): three posting
segments built in appends, so that no doc_base but the first is a
multiple of 32; every document a different length, so that non-zero
BM25 scores differ; a few marker terms with known document sets for the
operands; dated, domain-tagged attributes and tombstones for the
filters that run in the same batch."""
from __future__ import annotations

import numpy as np
import torch

from infomesh_amd.index.doc_attrs import DocFilter, TermOps, pack_attrs

SEGS = (45, 300, 200)            # doc_base 0, 45, 345
N_DOCS = sum(SEGS)
DIM = 32
GID0 = 7000
T0 = 1_700_000_000
LANGS = ["en", "de", "fr"]
DOMAINS = ["a.org", "b.org", "c.org", "d.org"]
DEAD = [GID0 + i for i in range(4, N_DOCS, 23)]

CONTENT_VOCAB = 60               # the scoring terms of the queries
FILLER = 50_000                  # length padding, never queried
# marker terms: where they occur is the test's ground truth
EVERY3, EVERY5, NOWHERE, EVERYWHERE, EDGES = 3000, 3001, 3002, 3003, 3004


def marker_docs() -> dict[int, set[int]]:
    first_last = set()
    base = 0
    for n in SEGS:               # first and last document of each segment
        first_last |= {base, base + n - 1}
        base += n
    return {EVERY3: set(range(0, N_DOCS, 3)),
            EVERY5: set(range(0, N_DOCS, 5)),
            NOWHERE: set(),
            EVERYWHERE: set(range(N_DOCS)),
            EDGES: first_last}


def corpus():
    """(tokens per document, (lang, domain, crawled_at) per document,
    bf16 unit embeddings)."""
    rng = np.random.default_rng(23)
    marks = marker_docs()
    toks = []
    for i in range(N_DOCS):
        content = rng.integers(0, CONTENT_VOCAB, size=rng.integers(8, 30))
        mine = [t for t, docs in marks.items() if i in docs]
        # length 40 + i exactly: all lengths differ
        pad = 40 + i - len(content) - len(mine)
        filler = FILLER + rng.integers(0, 8, size=pad)
        toks.append(np.concatenate([content, mine, filler]).astype(np.int64))
    meta = [(LANGS[i % 3], DOMAINS[(i // 3) % 4], T0 + i)
            for i in range(N_DOCS)]
    emb = torch.nn.functional.normalize(
        torch.randn(N_DOCS, DIM, generator=torch.Generator().manual_seed(23)),
        dim=-1).bfloat16()
    return toks, meta, emb


def build_shard(cls, toks, meta, emb, **kw):
    shard = cls(**kw)
    lo = 0
    for n in SEGS:
        for i in range(lo, lo + n):
            shard.add_document(GID0 + i, toks[i], emb[i],
                               attrs=pack_attrs(*meta[i]))
        shard.build()
        lo += n
    assert [s.doc_base for s in shard.segments] == [0, 45, 345]
    assert shard.delete(DEAD) == len(DEAD)
    return shard


def queries():
    """(scoring terms, bf16-representable unit embeddings, filters,
    term_ops) of one batch: operators alone, with a filter, with a
    domain list, and a row with neither."""
    rng = np.random.default_rng(29)
    terms = [rng.integers(0, CONTENT_VOCAB, size=4).astype(np.int64)
             for _ in range(6)]
    q = torch.nn.functional.normalize(
        torch.randn(6, DIM, generator=torch.Generator().manual_seed(29)),
        dim=-1).bfloat16().float()
    filters = [None,
               DocFilter(language="de"),
               DocFilter(exclude_sites=("b.org",), after=T0 + 50.5),
               None,
               DocFilter(sites=("a.org", "c.org")),
               None]
    ops = [TermOps.of(exclude=[EVERY3]),
           TermOps.of(require=[EVERY5], exclude=[EVERY3]),
           TermOps.of(require=[EVERY3, EVERYWHERE]),
           None,
           None,
           TermOps.of(require=[EDGES])]
    return terms, q, filters, ops


# Two shards' scores agree to SCORE_ATOL (the tolerance
# tests/test_doc_filter_gpu.py holds GpuShard to against CpuShard), so
# two documents can change places only when the oracle scores them
# within twice that of each other: such neighbours count as tied.
SCORE_ATOL = 1e-4
TIE = 2 * SCORE_ATOL
MAX_TIED = 0.10                  # of the returned positions of a test
K_CMP = 20                       # the k of the GpuShard / CpuShard comparison


def untied(want_scores: torch.Tensor, k: int) -> tuple[torch.Tensor, float]:
    """want_scores [B, k+1], descending, -inf padded -> (bool [B, k]:
    positions whose id must match, share of returned positions that are
    tied). A padded position (-inf) must match: its id is -1."""
    s = want_scores.double()
    gap = (s[:, :-1] - s[:, 1:]) > TIE                    # nan -> False
    ok = gap.clone()
    ok[:, 1:] &= gap[:, :-1]
    returned = torch.isfinite(s[:, :k])
    tied = (~ok & returned).sum().item() / max(returned.sum().item(), 1)
    return ok | ~returned, tied


def passes(gid: int, meta, f: DocFilter | None, t: TermOps | None,
           token_sets) -> bool:
    """Brute force: is this document live, inside the filter, and does
    its token set hold every required and no excluded id?"""
    i = gid - GID0
    lang, dom, crawled = meta[i]
    if gid in set(DEAD):
        return False
    if f is not None:
        if f.language and f.language != lang:
            return False
        if f.sites and dom not in f.sites:
            return False
        if dom in f.exclude_sites:
            return False
        if f.after is not None and crawled < np.ceil(f.after):
            return False
    if t is not None:
        if not set(t.require) <= token_sets[i]:
            return False
        if set(t.exclude) & token_sets[i]:
            return False
    return True
