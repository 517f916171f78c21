"""Plain-PyTorch fp32 reference implementations of every HIP kernel.

These are the numerics oracle for the GPU parity tests (SURVEY.md §4:
kernel-vs-CPU-reference strategy) and the executable spec of each op.
They are NOT used on the GPU path.
"""
from __future__ import annotations

import torch


def gemm_nt(a: torch.Tensor, b: torch.Tensor,
            bias: torch.Tensor | None = None, act: str = "none",
            alpha: float = 1.0) -> torch.Tensor:
    out = alpha * torch.matmul(a.float(), b.float().transpose(-1, -2))
    if bias is not None:
        out = out + bias.float()
    return apply_act(out, act)


def apply_act(x: torch.Tensor, act: str) -> torch.Tensor:
    if act == "gelu":
        return torch.nn.functional.gelu(x, approximate="tanh")
    if act == "silu":
        return torch.nn.functional.silu(x)
    if act == "relu":
        return torch.relu(x)
    if act == "tanh":
        return torch.tanh(x)
    return x


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
              residual: torch.Tensor | None = None,
              eps: float = 1e-12) -> torch.Tensor:
    xf = x.float()
    if residual is not None:
        xf = xf + residual.float()
    return torch.nn.functional.layer_norm(
        xf, (x.shape[-1],), gamma.float(), beta.float(), eps)


def rmsnorm(x: torch.Tensor, gamma: torch.Tensor,
            residual: torch.Tensor | None = None,
            eps: float = 1e-5) -> torch.Tensor:
    xf = x.float()
    if residual is not None:
        xf = xf + residual.float()
    var = xf.pow(2).mean(-1, keepdim=True)
    return xf * torch.rsqrt(var + eps) * gamma.float()


def softmax(scores: torch.Tensor, scale: float = 1.0, causal: bool = False,
            valid_len: torch.Tensor | None = None) -> torch.Tensor:
    G, Sq, Sk = scores.shape
    s = scores.float() * scale
    mask = torch.zeros_like(s, dtype=torch.bool)
    if causal:
        i = torch.arange(Sq).unsqueeze(1)
        j = torch.arange(Sk).unsqueeze(0)
        mask |= (j > i + (Sk - Sq)).unsqueeze(0)
    if valid_len is not None:
        j = torch.arange(Sk).view(1, 1, Sk)
        mask |= j >= valid_len.view(G, 1, 1)
    s = s.masked_fill(mask, float("-inf"))
    out = torch.softmax(s, dim=-1)
    return torch.nan_to_num(out, nan=0.0)  # fully-masked rows -> 0


def silu_mul(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    return torch.nn.functional.silu(gate.float()) * up.float()


def rope(x: torch.Tensor, cos_t: torch.Tensor, sin_t: torch.Tensor,
         pos: torch.Tensor, rot_dim: int | None = None) -> torch.Tensor:
    """NeoX half-rotation: pairs (d, d+rot/2)."""
    rows, H, D = x.shape
    rot = rot_dim or D
    half = rot // 2
    xf = x.float().clone()
    c = cos_t[pos.long()].view(rows, 1, half)
    s = sin_t[pos.long()].view(rows, 1, half)
    x0 = xf[..., :half].clone()
    x1 = xf[..., half:rot].clone()
    xf[..., :half] = x0 * c - x1 * s
    xf[..., half:rot] = x0 * s + x1 * c
    return xf


def pool(x: torch.Tensor, lens: torch.Tensor | None = None,
         mode: str = "cls", l2: bool = True) -> torch.Tensor:
    B, S, H = x.shape
    xf = x.float()
    if mode == "cls":
        out = xf[:, 0, :]
    else:
        if lens is None:
            out = xf.mean(1)
        else:
            mask = (torch.arange(S, device=x.device).view(1, S, 1)
                    < lens.view(B, 1, 1)).float()
            out = (xf * mask).sum(1) / mask.sum(1).clamp(min=1)
    if l2:
        out = torch.nn.functional.normalize(out, dim=-1)
    return out


def bm25_scores(postings: dict[int, list[tuple[int, int]]],
                doc_lens: torch.Tensor, queries: list[list[int]],
                n_docs: int, k1: float = 1.2, b: float = 0.75
                ) -> torch.Tensor:
    """Okapi BM25 over a {term: [(doc, tf)]} dict — the scalar spec of
    the CSR kernel. idf = ln(1 + (N - df + .5)/(df + .5))."""
    import math
    avgdl = float(doc_lens.float().mean()) if n_docs else 1.0
    norm = k1 * (1 - b + b * doc_lens.float() / avgdl)
    out = torch.zeros((len(queries), n_docs))
    for qi, terms in enumerate(queries):
        for t in terms:
            plist = postings.get(t, [])
            if not plist:
                continue
            df = len(plist)
            idf = math.log(1.0 + (n_docs - df + 0.5) / (df + 0.5))
            for doc, tf in plist:
                out[qi, doc] += idf * tf * (k1 + 1) / (tf + float(norm[doc]))
    return out


def simhash_fingerprint(hashes_per_doc: list[list[int]]) -> list[int]:
    """Charikar bit-vote over 64-bit shingle hashes."""
    fps = []
    for hashes in hashes_per_doc:
        fp = 0
        for bit in range(64):
            vote = sum(1 if (h >> bit) & 1 else -1 for h in hashes)
            if vote > 0:
                fp |= 1 << bit
        fps.append(fp)
    return fps


def hamming_matches(queries: list[int], table: list[int],
                    radius: int = 3) -> set[tuple[int, int]]:
    out = set()
    for m, q in enumerate(queries):
        for n, t in enumerate(table):
            if bin(q ^ t).count("1") <= radius:
                out.add((m, n))
    return out


def filter_bitmask(attrs: torch.Tensor, preds: torch.Tensor) -> torch.Tensor:
    """Oracle of csrc/docfilter.hip: attrs [N, 4] i32, preds [P, 4] i32
    -> pass bits [P, W] i32, W = ceil(N/64)*2, zero at positions >= N."""
    import numpy as np
    from ..index.doc_attrs import passes
    a = attrs.cpu().numpy()
    N = a.shape[0]
    W = (N + 63) // 64 * 2
    rows = []
    for pred in preds.cpu().numpy().view(np.uint32):
        ok = np.zeros(W * 32, dtype=bool)
        ok[:N] = passes(a, pred)
        rows.append(np.packbits(ok, bitorder="little").view(np.uint32))
    return torch.from_numpy(np.stack(rows).view(np.int32).reshape(-1, W))


def filter_bitmask_sets(attrs: torch.Tensor, preds: torch.Tensor,
                        desc: torch.Tensor, doms: torch.Tensor
                        ) -> torch.Tensor:
    """Oracle of filter_bitmask_sets: filter_bitmask plus, per predicate,
    the allow list doms[allow_off : allow_off + allow_n] and the block
    list doms[block_off : block_off + block_n] of desc [P, 4]."""
    import numpy as np
    from ..index.doc_attrs import passes
    a = attrs.cpu().numpy()
    h = doms.cpu().numpy().view(np.uint32)
    N = a.shape[0]
    W = (N + 63) // 64 * 2
    rows = []
    for pred, (ao, an, bo, bn) in zip(preds.cpu().numpy().view(np.uint32),
                                      desc.cpu().numpy().tolist()):
        ok = np.zeros(W * 32, dtype=bool)
        ok[:N] = passes(a, pred, allow=h[ao:ao + an], block=h[bo:bo + bn])
        rows.append(np.packbits(ok, bitorder="little").view(np.uint32))
    return torch.from_numpy(np.stack(rows).view(np.int32).reshape(-1, W))


def term_bitmask(base_bits: torch.Tensor, src_row: torch.Tensor,
                 segments, op_off: torch.Tensor, op_kind: torch.Tensor,
                 N: int) -> torch.Tensor:
    """Oracle of csrc/termmask.hip, same signature as
    kernels.term_bitmask: plain set arithmetic over the posting arrays.
    Row r starts from base_bits[src_row[r]]; inside every segment's
    document range a document keeps its bit iff it is in the posting
    set of every require operand (kind 0) and of no exclude operand
    (kind 1). Documents outside every segment keep their base bit."""
    import numpy as np
    W = (N + 63) // 64 * 2
    words = base_bits.cpu().numpy().view(np.uint32)
    base_ok = np.unpackbits(words.view(np.uint8), axis=1,
                            bitorder="little").astype(bool)     # [P, W*32]
    off = op_off.cpu().numpy().astype(np.int64)
    kind = op_kind.cpu().numpy()
    rows = []
    for r, p in enumerate(src_row.cpu().numpy().astype(np.int64)):
        ok = base_ok[p].copy()
        for doc_ids, doc_base, nseg, op_begin, op_end in segments:
            ids = doc_ids.cpu().numpy().astype(np.int64)
            begin = op_begin.cpu().numpy()
            end = op_end.cpu().numpy()
            in_seg = np.arange(doc_base, doc_base + nseg)
            keep = np.ones(nseg, dtype=bool)
            for t in range(off[r], off[r + 1]):
                has = np.isin(in_seg, ids[begin[t]:end[t]] + doc_base)
                keep &= ~has if kind[t] else has
            ok[doc_base:doc_base + nseg] &= keep
        rows.append(np.packbits(ok, bitorder="little").view(np.uint32))
    return torch.from_numpy(np.stack(rows).view(np.int32).reshape(-1, W))


def facet_counts(scores: torch.Tensor, rows: torch.Tensor,
                 attrs: torch.Tensor, edges: torch.Tensor,
                 langs: torch.Tensor, dom_desc: torch.Tensor,
                 doms: torch.Tensor, mask: torch.Tensor | None = None,
                 row_pred: torch.Tensor | None = None) -> torch.Tensor:
    """Oracle of csrc/facets.hip, same arguments as kernels.facet_counts:
    document d matches batch row b = rows[r] iff its bit is set in
    mask[row_pred[b]] (no mask: every document) and scores[b, d] > 0; a
    match adds 1 to TOTAL, to one date slot, to one language slot and to
    at most one domain slot of counts[r]. The rules are written in numpy
    once, in index/doc_attrs.facet_counts_np, which CpuShard counts
    with as well; this function only unpacks the kernel's arguments
    (bit rows, descriptors) for it. Returns counts [R, F] i32."""
    import numpy as np
    from ..index.doc_attrs import PackedFacets, facet_counts_np
    s = scores.detach().float().cpu().numpy()
    B, N = s.shape
    h = doms.cpu().numpy().view(np.uint32)
    desc = dom_desc.cpu().numpy().astype(np.int64).reshape(-1, 2)
    packed = PackedFacets(
        edges=tuple(int(v) for v in edges.cpu().numpy().view(np.uint32)),
        langs=tuple(int(v) for v in langs.cpu().numpy().view(np.uint32)),
        rows=tuple(int(b) for b in rows.cpu().numpy()),
        lists=tuple(tuple(int(v) for v in h[off:off + n])
                    for off, n in desc))
    return torch.from_numpy(facet_counts_np(
        s, _fail_rows(mask, row_pred, N), attrs.cpu().numpy(), packed))


def _fail_rows(mask, row_pred, N: int):
    """bool [B, N], True where a document fails its row's mask; None
    without a mask."""
    import numpy as np
    if mask is None:
        return None
    words = mask.cpu().numpy().view(np.uint32)
    ok = np.unpackbits(words.view(np.uint8), axis=1,
                       bitorder="little")[:, :N].astype(bool)
    return ~ok[row_pred.cpu().numpy().astype(np.int64)]


def domain_count(scores: torch.Tensor, rows: torch.Tensor,
                 dom_id: torch.Tensor, D: int,
                 mask: torch.Tensor | None = None,
                 row_pred: torch.Tensor | None = None,
                 out: torch.Tensor | None = None) -> torch.Tensor:
    """Oracle of csrc/domtop.hip's domain_count, same arguments as
    kernels.domain_count: cnt[r, i] = the matching documents of batch
    row rows[r] (facet_counts' rule) whose dom_id is i. [R, D] i32."""
    import numpy as np
    s = scores.detach().float().cpu().numpy()
    fail = _fail_rows(mask, row_pred, s.shape[1])
    ids = dom_id.cpu().numpy().astype(np.int64)
    cnt = np.zeros((rows.numel(), D), dtype=np.int64)
    for r, b in enumerate(rows.cpu().numpy()):
        m = s[b] > 0
        if fail is not None:
            m &= ~fail[b]
        cnt[r] = np.bincount(ids[m], minlength=D)
    return torch.from_numpy(cnt.astype(np.int32))


def domain_select(cnt: torch.Tensor, dom_keys: torch.Tensor,
                  K: int) -> torch.Tensor:
    """Oracle of csrc/domtop.hip's domain_select, same arguments as
    kernels.domain_select: per row the non-zero counts by count
    descending, then hash ascending as unsigned (np.lexsort, as
    index/doc_attrs.domain_top_np orders them), the first K as (hash
    bits, count) pairs, (0, 0) behind them. [R, K, 2] i32."""
    import numpy as np
    c = cnt.cpu().numpy().astype(np.int64)
    keys = dom_keys.cpu().numpy().view(np.uint32).astype(np.int64)
    R, D = c.shape
    out = np.zeros((R, K, 2), dtype=np.int64)
    for r in range(R):
        nz = np.nonzero(c[r])[0]
        order = nz[np.lexsort((keys[nz], -c[r, nz]))][:K]
        out[r, :len(order), 0] = keys[order]
        out[r, :len(order), 1] = c[r, order]
    return torch.from_numpy(out.astype(np.uint32).view(np.int32))


def domain_top(scores: torch.Tensor, rows: torch.Tensor,
               attrs: torch.Tensor, K: int,
               mask: torch.Tensor | None = None,
               row_pred: torch.Tensor | None = None) -> torch.Tensor:
    """Oracle of domain_count followed by domain_select over a shard's
    attribute records, with the kernels' arguments: the rules are
    written once, in index/doc_attrs.domain_top_np, which CpuShard uses
    as well; this function only unpacks the mask for it. [R, K, 2] i32."""
    from ..index.doc_attrs import domain_top_np
    s = scores.detach().float().cpu().numpy()
    return torch.from_numpy(domain_top_np(
        s, _fail_rows(mask, row_pred, s.shape[1]), attrs.cpu().numpy(),
        [int(b) for b in rows.cpu().numpy()], K))


def collapse_topk(scores: torch.Tensor, rows: torch.Tensor,
                  dom_id: torch.Tensor, m: int, k: int, positive: bool,
                  mask: torch.Tensor | None = None,
                  row_pred: torch.Tensor | None = None
                  ) -> tuple[torch.Tensor, torch.Tensor]:
    """Oracle of csrc/collapse.hip (domain_best x m, then
    collapse_select), by sorting and counting: per batch row rows[r],
    the eligible documents (they pass the mask; positive: and score > 0)
    sorted by ordered_key(score) descending, then column ascending; a
    document stays if fewer than m documents of its dom_id stand before
    it; the first k of those, padded with -inf / -1.
    -> (vals [R, k] f32, idx [R, k] i32)."""
    s = scores.detach().float().cpu()
    return collapse_topk_rows(
        s, _fail_rows(mask, row_pred, s.shape[1]), dom_id,
        [int(b) for b in rows.cpu().numpy()], m, k, positive)


def collapse_topk_rows(s: torch.Tensor, fail, dom_id: torch.Tensor,
                       rows: list[int], m: int, k: int, positive: bool
                       ) -> tuple[torch.Tensor, torch.Tensor]:
    """collapse_topk with the mask unpacked: s [B, N] f32 on the host,
    fail bool [B, N] (numpy, True where a document fails its row's mask)
    or None. CpuShard calls this with the fail rows it has."""
    import numpy as np
    okey = ordered_key(s).numpy()
    s = s.numpy()
    N = s.shape[1]
    dom = dom_id.cpu().numpy().astype(np.int64)
    R = len(rows)
    vals = np.full((R, k), -np.inf, dtype=np.float32)
    idx = np.full((R, k), -1, dtype=np.int32)
    for r, b in enumerate(rows):
        ok = s[b] > 0 if positive else np.ones(N, dtype=bool)
        if fail is not None:
            ok = ok & ~fail[b]
        cols = np.nonzero(ok)[0]
        cols = cols[np.lexsort((cols, -okey[b, cols]))]
        # rank within the domain: group the ordered list by domain,
        # stably, and count from each group's start
        d = dom[cols]
        by_dom = np.argsort(d, kind="stable")
        ds = d[by_dom]
        rank = np.empty(len(cols), dtype=np.int64)
        rank[by_dom] = np.arange(len(cols)) - np.searchsorted(ds, ds)
        keep = cols[rank < m][:k]
        vals[r, :len(keep)] = s[b, keep]
        idx[r, :len(keep)] = keep
    return torch.from_numpy(vals), torch.from_numpy(idx)


def masked_topk(scores: torch.Tensor, k: int, bits: torch.Tensor,
                row_pred: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """Oracle of the masked top-k: failing columns become -inf, then
    torch.topk; -inf results carry index -1."""
    import numpy as np
    B, N = scores.shape
    words = bits.cpu().numpy().view(np.uint32)
    ok = np.unpackbits(words.view(np.uint8), axis=1,
                       bitorder="little")[:, :N].astype(bool)
    ok = torch.from_numpy(ok[row_pred.cpu().numpy().astype(np.int64)])
    s = scores.detach().float().cpu().masked_fill(~ok, float("-inf"))
    vals, idx = torch.topk(s, k, dim=1)
    idx = torch.where(torch.isinf(vals) & (vals < 0),
                      torch.full_like(idx, -1), idx)
    return vals, idx


def ordered_key(x: torch.Tensor) -> torch.Tensor:
    """float_to_ordered of csrc/common.h as int64: the total order the
    selector ranks f32 by (-0.0 just below +0.0, -inf lowest non-NaN)."""
    bits = x.detach().float().cpu().contiguous().view(torch.int32) \
        .to(torch.int64) & 0xFFFFFFFF
    return torch.where(bits >= 0x80000000, bits ^ 0xFFFFFFFF,
                       bits | 0x80000000)


def block_max(scores: torch.Tensor, W: int) -> torch.Tensor:
    """Oracle of the GEMM's block maxima: [B, N] f32 -> [B, ceil(N/W)],
    the maximum in ordered_key order of every W consecutive columns
    (the last block over its valid columns only), bit for bit."""
    s = scores.detach().float().cpu()
    B, N = s.shape
    NB = (N + W - 1) // W
    key = torch.full((B, NB * W), -1, dtype=torch.int64)
    key[:, :N] = ordered_key(s)
    pos = key.view(B, NB, W).argmax(dim=2)
    cols = (pos + torch.arange(NB) * W).clamp(max=N - 1)
    return s.gather(1, cols)


def topk_pruned(scores: torch.Tensor, bmax: torch.Tensor, W: int,
                k: int) -> tuple[torch.Tensor, torch.Tensor]:
    """Oracle of infomesh_topk_pruned, by the same steps: take the
    min(k, NB) blocks with the largest maxima, and the top k of their
    union in value order, equal values by ascending column. Rows with
    fewer than k columns pad with -inf / -1."""
    s = scores.detach().float().cpu()
    B, N = s.shape
    NB = (N + W - 1) // W
    assert bmax.shape == (B, NB)
    k1 = min(k, NB)
    ids = torch.topk(ordered_key(bmax), k1, dim=1).indices.sort(dim=1).values
    cols = (ids[:, :, None] * W + torch.arange(W)).reshape(B, k1 * W)
    real = cols < N
    cand = s.gather(1, cols.clamp(max=N - 1))
    # padding ranks under everything, a real -inf included
    key = torch.where(real, ordered_key(cand), torch.full_like(cols, -1))
    # +-0.0 are one value when it comes to the order among equals
    key = torch.where(key == 0x7FFFFFFF, key + 1, key)
    order = torch.sort(key, dim=1, descending=True, stable=True).indices
    kk = min(k, k1 * W)
    order = order[:, :kk]
    vals = torch.full((B, k), float("-inf"))
    idx = torch.full((B, k), -1, dtype=torch.int64)
    ok = real.gather(1, order)
    vals[:, :kk] = torch.where(ok, cand.gather(1, order), vals[:, :kk])
    idx[:, :kk] = torch.where(ok, cols.gather(1, order), idx[:, :kk])
    return vals, idx


def attn_decode(q: torch.Tensor, k_cache: torch.Tensor,
                v_cache: torch.Tensor, lens: torch.Tensor,
                scale: float) -> torch.Tensor:
    B, H, D = q.shape
    _, Hkv, Smax, _ = k_cache.shape
    group = H // Hkv
    out = torch.zeros_like(q, dtype=torch.float32)
    for b in range(B):
        L = int(lens[b])
        for h in range(H):
            kv = h // group
            k = k_cache[b, kv, :L].float()
            v = v_cache[b, kv, :L].float()
            p = torch.softmax(q[b, h].float() @ k.T * scale, dim=-1)
            out[b, h] = p @ v
    return out
