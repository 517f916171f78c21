"""GPU kernel parity tests vs the fp32 PyTorch references (MI355X only).

Strategy: every HIP kernel is compared against
ops/reference.py on random data; GEMM/attention inputs are asymmetric so
operand/output transposes cannot pass (guide §5.4 rule 16).
"""
from __future__ import annotations

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from infomesh_amd.ops import _build
    _build.build()
from infomesh_amd.ops import kernels as K
from infomesh_amd.ops import reference as R


def _skip_no_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(autouse=True)
def _gpu():
    _skip_no_gpu()
    torch.manual_seed(0)


def _assert_close(gpu, ref, rtol=2e-2, atol=2e-2, what=""):
    gpu = gpu.float().cpu()
    ref = ref.float().cpu()
    err = (gpu - ref).abs().max().item()
    scale = ref.abs().max().item() + 1e-6
    assert err <= atol + rtol * scale, f"{what}: max err {err} (scale {scale})"


# ------------------------------------------------------------------- GEMM

@pytest.mark.parametrize("M,N,Kd", [
    (128, 128, 64), (64, 384, 384), (200, 1000, 96),
    (256, 1536, 384), (33, 100, 32), (512, 512, 512),
    (64, 1000, 96), (17, 384, 64), (64, 200, 32), (32, 4096, 384),
])
def test_gemm_nt_shapes(M, N, Kd):
    a = torch.randn(M, Kd, device="cuda").bfloat16()
    b = torch.randn(N, Kd, device="cuda").bfloat16()
    out = K.gemm_nt(a, b)
    ref = R.gemm_nt(a.cpu(), b.cpu())
    _assert_close(out, ref, rtol=3e-2, atol=Kd ** 0.5 * 2e-2,
                  what=f"gemm {M}x{N}x{Kd}")


@pytest.mark.parametrize("M,N,Kd,bias_silu,out_f32,tile", [
    # 128^2, BK=64, full tiles: the LDS-staged f32 epilogue
    (128, 256, 2112, False, True, (128, 128, 64, False)),
    # 128^2, BK=64, partial tiles
    (130, 200, 2112, True, False, (128, 128, 64, False)),
    # 128^2, BK=32
    (130, 200, 2080, False, False, (128, 128, 32, False)),
    # 64x128, BK=64, staged f32
    (64, 256, 128, False, True, (64, 128, 64, False)),
    # pipelined 64^2, three K-steps: all three buffers rotate
    (192, 192, 192, False, False, (64, 64, 64, True)),
    # M <= 64 takes the 64x128 tile, never the pipelined one
    (64, 64, 64, False, False, (64, 128, 64, False)),
])
def test_gemm_tile_variants(M, N, Kd, bias_silu, out_f32, tile):
    """One case per gemm.hip kernel variant the other tests do not pin;
    the tile assertion keeps a heuristics change from moving a case to
    another kernel unnoticed."""
    assert K.gemm_route(M, N, Kd, 1) == "gemm"
    assert K.gemm_tile(M, N, Kd, 1) == tile
    a = torch.randn(M, Kd, device="cuda").bfloat16()
    b = torch.randn(N, Kd, device="cuda").bfloat16()
    bias = torch.randn(N, device="cuda") if bias_silu else None
    act = "silu" if bias_silu else "none"
    out = K.gemm_nt(a, b, bias=bias, act=act, out_f32=out_f32)
    assert out.dtype == (torch.float32 if out_f32 else torch.bfloat16)
    ref = R.gemm_nt(a.cpu(), b.cpu(),
                    bias.cpu() if bias_silu else None, act=act)
    _assert_close(out, ref, rtol=3e-2, atol=Kd ** 0.5 * 2e-2,
                  what=f"gemm {M}x{N}x{Kd} tile {tile}")


@pytest.mark.parametrize("M,N,Kd", [(1, 9216, 3072), (4, 100, 64),
                                    (16, 32064, 3072), (8, 3072, 8192)])
def test_gemv_skinny_m(M, N, Kd):
    """M<=16 dispatches to the wave-per-column GEMV kernel."""
    a = torch.randn(M, Kd, device="cuda").bfloat16()
    b = torch.randn(N, Kd, device="cuda").bfloat16()
    bias = torch.randn(N, device="cuda")
    out = K.gemm_nt(a, b, bias=bias, act="silu", out_f32=True)
    ref = R.gemm_nt(a.cpu(), b.cpu(), bias.cpu(), act="silu")
    _assert_close(out, ref, rtol=3e-2, atol=Kd ** 0.5 * 2e-2,
                  what=f"gemv {M}x{N}x{Kd}")


def test_gemv_batched():
    G, M, N, Kd = 5, 2, 64, 96
    a = torch.randn(G, M, Kd, device="cuda").bfloat16()
    b = torch.randn(G, N, Kd, device="cuda").bfloat16()
    out = K.gemm_nt(a, b)
    _assert_close(out, R.gemm_nt(a.cpu(), b.cpu()), what="gemv batched")


def test_gemm_asymmetric_catches_transpose():
    # Asymmetric B (guide: A=I with asymmetric B catches row/col swap).
    M = N = Kd = 128
    a = torch.eye(M, device="cuda").bfloat16()
    b = torch.arange(N * Kd, device="cuda").reshape(N, Kd).bfloat16() / (N * Kd)
    out = K.gemm_nt(a, b)
    ref = R.gemm_nt(a.cpu(), b.cpu())
    _assert_close(out, ref, what="gemm transpose check")


def test_gemm_bias_act_f32out():
    a = torch.randn(96, 64, device="cuda").bfloat16()
    b = torch.randn(256, 64, device="cuda").bfloat16()
    bias = torch.randn(256, device="cuda")
    for act in ("none", "gelu", "silu", "relu", "tanh"):
        out = K.gemm_nt(a, b, bias=bias, act=act, out_f32=True)
        assert out.dtype == torch.float32
        ref = R.gemm_nt(a.cpu(), b.cpu(), bias.cpu(), act=act)
        _assert_close(out, ref, what=f"gemm act={act}")


def test_gemm_batched_and_shared_b():
    G, M, N, Kd = 6, 64, 96, 64
    a = torch.randn(G, M, Kd, device="cuda").bfloat16()
    b = torch.randn(G, N, Kd, device="cuda").bfloat16()
    out = K.gemm_nt(a, b)
    ref = R.gemm_nt(a.cpu(), b.cpu())
    _assert_close(out, ref, what="batched gemm")
    bs = torch.randn(N, Kd, device="cuda").bfloat16()
    out2 = K.gemm_nt(a, bs)
    ref2 = R.gemm_nt(a.cpu(), bs.cpu())
    _assert_close(out2, ref2, what="shared-B gemm")


def test_gemm_alpha():
    a = torch.randn(64, 32, device="cuda").bfloat16()
    b = torch.randn(64, 32, device="cuda").bfloat16()
    out = K.gemm_nt(a, b, alpha=0.125, out_f32=True)
    _assert_close(out, R.gemm_nt(a.cpu(), b.cpu(), alpha=0.125), what="alpha")


# ------------------------------------------------------------------ norms

def test_layernorm():
    x = torch.randn(37, 384, device="cuda").bfloat16()
    g = torch.randn(384, device="cuda").bfloat16()
    b = torch.randn(384, device="cuda").bfloat16()
    _assert_close(K.layernorm(x, g, b),
                  R.layernorm(x.cpu(), g.cpu(), b.cpu()), what="ln")


def test_layernorm_residual():
    x = torch.randn(16, 768, device="cuda").bfloat16()
    r = torch.randn(16, 768, device="cuda").bfloat16()
    g = torch.randn(768, device="cuda").bfloat16()
    b = torch.randn(768, device="cuda").bfloat16()
    out, res = K.layernorm(x, g, b, residual=r, return_residual=True)
    _assert_close(out, R.layernorm(x.cpu(), g.cpu(), b.cpu(), r.cpu()),
                  what="ln+res")
    _assert_close(res, x.cpu().float() + r.cpu().float(), what="res out")


def test_layernorm_huge_row():
    x = torch.randn(3, 32768, device="cuda").bfloat16()  # beyond MAXV regs
    g = torch.ones(32768, device="cuda").bfloat16()
    b = torch.zeros(32768, device="cuda").bfloat16()
    _assert_close(K.layernorm(x, g, b),
                  R.layernorm(x.cpu(), g.cpu(), b.cpu()), what="ln huge")


def test_rmsnorm():
    x = torch.randn(21, 3072, device="cuda").bfloat16()
    g = torch.randn(3072, device="cuda").bfloat16()
    _assert_close(K.rmsnorm(x, g), R.rmsnorm(x.cpu(), g.cpu()), what="rms")


# ---------------------------------------------------------------- softmax

def test_softmax_plain_and_scale():
    s = torch.randn(4, 32, 200, device="cuda")
    _assert_close(K.softmax(s, scale=0.3), R.softmax(s.cpu(), scale=0.3),
                  atol=5e-3, what="softmax")


def test_softmax_causal():
    s = torch.randn(2, 64, 64, device="cuda")
    _assert_close(K.softmax(s, causal=True), R.softmax(s.cpu(), causal=True),
                  atol=5e-3, what="softmax causal")


def test_softmax_causal_prefill_offset():
    s = torch.randn(2, 16, 48, device="cuda")  # Sq < Sk (continuation)
    _assert_close(K.softmax(s, causal=True), R.softmax(s.cpu(), causal=True),
                  atol=5e-3, what="softmax causal offset")


def test_softmax_valid_len():
    s = torch.randn(3, 8, 100, device="cuda")
    vl = torch.tensor([10, 100, 1], device="cuda", dtype=torch.int32)
    _assert_close(K.softmax(s, valid_len=vl),
                  R.softmax(s.cpu(), valid_len=vl.cpu()),
                  atol=5e-3, what="softmax masked")


# ------------------------------------------------------------ elementwise

def test_bias_act_inplace():
    x = torch.randn(10, 64, device="cuda").bfloat16()
    b = torch.randn(64, device="cuda")
    ref = R.apply_act(x.cpu().float() + b.cpu(), "gelu")
    _assert_close(K.bias_act(x, b, "gelu"), ref, what="bias_gelu")


def test_silu_mul_and_add():
    g = torch.randn(8, 512, device="cuda").bfloat16()
    u = torch.randn(8, 512, device="cuda").bfloat16()
    _assert_close(K.silu_mul(g, u), R.silu_mul(g.cpu(), u.cpu()), what="swiglu")
    _assert_close(K.add(g, u), g.cpu().float() + u.cpu().float(), what="add")


def test_rope():
    rows, H, D = 6, 4, 96
    x = torch.randn(rows, H, D, device="cuda").bfloat16()
    inv = 1.0 / (10000 ** (torch.arange(D // 2).float() * 2 / D))
    t = torch.arange(64).float()
    ang = torch.outer(t, inv)
    cos_t, sin_t = ang.cos().cuda(), ang.sin().cuda()
    pos = torch.tensor([0, 5, 9, 13, 33, 63], device="cuda", dtype=torch.int32)
    ref = R.rope(x.cpu(), cos_t.cpu(), sin_t.cpu(), pos.cpu())
    _assert_close(K.rope(x, cos_t, sin_t, pos), ref, what="rope")


def test_gather():
    table = torch.randn(1000, 384, device="cuda").bfloat16()
    ids = torch.randint(0, 1000, (57,), device="cuda", dtype=torch.int32)
    _assert_close(K.gather(table, ids),
                  table.cpu()[ids.cpu().long()].float(), what="gather")


def test_pool_cls_and_mean():
    x = torch.randn(5, 33, 384, device="cuda").bfloat16()
    lens = torch.tensor([33, 10, 1, 20, 5], device="cuda", dtype=torch.int32)
    _assert_close(K.pool(x, mode="cls"), R.pool(x.cpu(), mode="cls"),
                  atol=1e-2, what="cls pool")
    _assert_close(K.pool(x, lens, mode="mean"),
                  R.pool(x.cpu(), lens.cpu(), mode="mean"),
                  atol=1e-2, what="mean pool")


def test_argmax():
    logits = torch.randn(17, 32064, device="cuda")
    out = K.argmax(logits)
    ref = logits.cpu().argmax(-1)
    assert (out.cpu().long() == ref).all()


# ------------------------------------------------------------------ top-k

@pytest.mark.parametrize("B,N,k", [(4, 10_000, 10), (2, 1_000_000, 100),
                                   (64, 50_000, 100), (1, 5000, 1024)])
def test_topk_matches_torch(B, N, k):
    scores = torch.randn(B, N, device="cuda")
    vals, idx = K.topk(scores, k)
    rv, ri = torch.topk(scores, k, dim=-1)
    assert torch.allclose(vals, rv, atol=0), \
        f"value mismatch: {(vals - rv).abs().max()}"
    # Indices must point at their values (ties may reorder).
    picked = torch.gather(scores, 1, idx.long())
    assert torch.allclose(picked, vals, atol=0)


def test_topk_negative_scores():
    scores = -torch.rand(3, 20_000, device="cuda") - 5.0
    vals, idx = K.topk(scores, 7)
    rv, _ = torch.topk(scores, 7, dim=-1)
    assert torch.allclose(vals, rv, atol=0)


# ------------------------------------------------------------------- BM25

def test_bm25_parity():
    import numpy as np
    rng = np.random.default_rng(0)
    n_docs, vocab = 5000, 300
    postings: dict[int, list[tuple[int, int]]] = {}
    doc_lens = torch.zeros(n_docs, dtype=torch.long)
    for t in range(vocab):
        df = int(rng.integers(1, 200))
        docs = rng.choice(n_docs, size=df, replace=False)
        plist = []
        for d in sorted(docs):
            tf = int(rng.integers(1, 5))
            plist.append((int(d), tf))
            doc_lens[d] += tf
        postings[t] = plist
    queries = [[1, 2, 3], [10, 250], [0], [299, 5, 5]]
    # engine semantics: query terms are DEDUPED per query (qtf dropped,
    # matching round-1 gpu_index dedupe + FTS5 MATCH behavior), so the
    # oracle gets the deduped lists
    ref = R.bm25_scores(postings, doc_lens,
                        [sorted(set(q)) for q in queries], n_docs)

    # Build segment CSR (doc ids asc per term, tf|dl packed) like
    # index/gpu_index.py _install_segment does.
    import math
    offsets = [0]
    doc_ids, tfdl = [], []
    for t in range(vocab):
        for d, tf in postings[t]:
            doc_ids.append(d)
            tfdl.append(tf | (int(doc_lens[d]) << 16))
        offsets.append(len(doc_ids))
    avgdl = float(doc_lens.float().mean())
    dev = "cuda"
    B = len(queries)
    # per-(q, term) tuple table (deduped per query, unique across
    # queries for the bounds pre-pass)
    import numpy as np2
    qrows, tlist = [], []
    for qi, terms in enumerate(queries):
        for t in sorted(set(terms)):
            qrows.append(qi); tlist.append(t)
    uterms, qt_ut = np2.unique(np2.array(tlist), return_inverse=True)
    qt_off = [0]
    qi_ = []
    for qi, terms in enumerate(queries):
        for t in sorted(set(terms)):
            df = offsets[t + 1] - offsets[t]
            qi_.append(math.log(1.0 + (n_docs - df + 0.5) / (df + 0.5)))
        qt_off.append(len(qi_))
    bd = 4096
    nblocks = (n_docs + bd - 1) // bd
    bounds = torch.empty(len(uterms) * nblocks * 2, dtype=torch.int32,
                         device=dev)
    # garbage-filled output: the kernel must write every column
    scores = torch.full((B, n_docs), float("nan"), device=dev)
    K.bm25_block(
        torch.tensor(doc_ids, dtype=torch.int32, device=dev),
        torch.tensor(tfdl, dtype=torch.int32, device=dev),
        torch.tensor(qt_off, dtype=torch.int32, device=dev),
        torch.from_numpy(qt_ut.astype(np2.int32)).to(dev),
        torch.tensor(qi_, dtype=torch.float32, device=dev),
        torch.from_numpy(np2.array([offsets[t] for t in uterms],
                                   dtype=np2.int64)).to(dev),
        torch.from_numpy(np2.array([offsets[t + 1] for t in uterms],
                                   dtype=np2.int64)).to(dev),
        bounds, scores, doc_base=0, nseg=n_docs, bd=bd, avgdl=avgdl)
    assert not torch.isnan(scores).any(), "kernel left columns unwritten"
    _assert_close(scores, ref, rtol=1e-3, atol=1e-3, what="bm25")


def test_bm25_scores_repeat_bit_for_bit():
    """A doc's term contributions are summed in a fixed order, so the
    same queries give the same scores and the same hit order on every
    run — bit for bit, also for docs matching three or more terms,
    where a racing f32 sum would move by an ulp. Shapes: more than one
    doc block, a doc count that is no multiple of the block, queries of
    1, 2, 5 and 12 terms (12 > the 4 waves of a workgroup)."""
    import numpy as np
    from infomesh_amd.index.synth import build_synth_shard
    shard = build_synth_shard(20_011, avg_len=60, device="cuda", seed=2,
                              with_dense=False)
    common = np.arange(0, 12, dtype=np.int64)      # Zipf head: dense hits
    queries = [common, common[:5], common[3:5], common[7:8],
               np.array([60, 3, 900, 1, 17], dtype=np.int64)]
    first = shard.search(queries, None, k=100)
    s0, i0 = first.bm25_scores.clone(), first.bm25_ids.clone()
    assert (i0[0] >= 0).all() and s0[0, 0] > s0[0, -1] > 0
    for _ in range(4):
        h = shard.search(queries, None, k=100)
        assert torch.equal(h.bm25_scores, s0)
        assert torch.equal(h.bm25_ids, i0)


def test_bm25_segmented_matches_merged():
    """Three appended segments (O(new) flush) vs one bulk build, and vs
    the post-optimize() merged segment — identical search results on the
    GPU kernels. Also covers BM25-only GpuShard.search() (the round-1
    dense-less branch NameError path)."""
    import numpy as np
    from infomesh_amd.index.gpu_index import GpuShard
    rng = np.random.default_rng(3)
    docs = [rng.integers(0, 4000, size=rng.integers(5, 60)).astype(np.int64)
            for _ in range(3000)]
    inc = GpuShard("cuda")
    start = 0
    for batch in (1200, 900, 900):
        for i in range(start, start + batch):
            inc.add_document(10_000 + i, docs[i], None)
        inc.build()
        start += batch
    assert len(inc.segments) == 3
    bulk = GpuShard("cuda")
    for i in range(3000):
        bulk.add_document(10_000 + i, docs[i], None)
    bulk.build()
    queries = [rng.integers(0, 4000, size=5).astype(np.int64)
               for _ in range(8)]
    hi = inc.search(queries, None, k=20)     # BM25-only branch
    hb = bulk.search(queries, None, k=20)
    # tie membership at rank k is arbitrary (the selector's accepted
    # semantics) — compare top-k VALUES, and require equal result counts
    _assert_close(hi.bm25_scores, hb.bm25_scores, rtol=1e-4, atol=1e-4,
                  what="seg-bm25")
    assert (hi.bm25_ids >= 0).sum() == (hb.bm25_ids >= 0).sum()
    inc.optimize()
    assert len(inc.segments) == 1
    ho = inc.search(queries, None, k=20)
    _assert_close(ho.bm25_scores, hb.bm25_scores, rtol=1e-4, atol=1e-4,
                  what="opt-bm25")


# ---------------------------------------------------------------- simhash

def test_simhash_fingerprint_parity():
    import numpy as np
    rng = np.random.default_rng(1)
    docs = [list(rng.integers(0, 2**63, size=int(rng.integers(1, 50))))
            for _ in range(100)]
    ref = R.simhash_fingerprint(docs)
    offsets = [0]
    flat = []
    for d in docs:
        flat.extend(d)
        offsets.append(len(flat))
    dev = "cuda"
    fps = K.simhash_fingerprint(
        torch.tensor(offsets, dtype=torch.int64, device=dev),
        torch.tensor(flat, dtype=torch.int64, device=dev))
    got = [int(v) & (2**64 - 1) for v in fps.cpu()]
    assert got == ref


def test_hamming_scan_parity():
    import numpy as np
    rng = np.random.default_rng(2)
    table = list(rng.integers(0, 2**63, size=2000))
    queries = [table[5], table[100] ^ 0b111, int(rng.integers(0, 2**63))]
    ref = R.hamming_matches(queries, table, radius=3)
    dev = "cuda"
    q, n, d = K.hamming_scan(
        torch.tensor(queries, dtype=torch.int64, device=dev),
        torch.tensor(table, dtype=torch.int64, device=dev), radius=3)
    got = set(zip(q.cpu().tolist(), n.cpu().tolist()))
    assert got == ref


# ------------------------------------------------------- fused attention

def _attn_ref(q, k, v, valid=None, causal=False, scale=None):
    B, nh, Sq, d = q.shape
    _, nhk, Sk, _ = k.shape
    rep = nh // nhk
    kf = k.float().repeat_interleave(rep, dim=1)
    vf = v.float().repeat_interleave(rep, dim=1)
    s = torch.einsum("bhqd,bhkd->bhqk", q.float(), kf) * (scale or d ** -0.5)
    mask = torch.zeros(B, 1, Sq, Sk, dtype=torch.bool)
    if causal:
        i = torch.arange(Sq).view(Sq, 1)
        j = torch.arange(Sk).view(1, Sk)
        mask = mask | (j > i + (Sk - Sq)).view(1, 1, Sq, Sk)
    if valid is not None:
        mask = mask | (torch.arange(Sk).view(1, 1, 1, Sk)
                       >= valid.view(B, 1, 1, 1))
    s = s.masked_fill(mask, float("-inf"))
    p = torch.nan_to_num(torch.softmax(s, -1), nan=0.0)
    return torch.einsum("bhqk,bhkd->bhqd", p, vf).reshape(B * nh, Sq, d)


@pytest.mark.parametrize("D", [32, 64, 96, 128])
def test_attn_fused_basic(D):
    B, nh, S = 2, 3, 80
    q = torch.randn(B, nh, S, D, device="cuda").bfloat16()
    k = torch.randn(B, nh, S, D, device="cuda").bfloat16()
    v = torch.randn(B, nh, S, D, device="cuda").bfloat16()
    out = K.attn_fused(q, k, v)
    ref = _attn_ref(q.cpu(), k.cpu(), v.cpu())
    _assert_close(out, ref, atol=3e-2, what=f"attn_fused D={D}")


def test_attn_fused_valid_len():
    B, nh, S, D = 3, 2, 100, 64
    q = torch.randn(B, nh, S, D, device="cuda").bfloat16()
    k = torch.randn(B, nh, S, D, device="cuda").bfloat16()
    v = torch.randn(B, nh, S, D, device="cuda").bfloat16()
    vl = torch.tensor([100, 17, 1], device="cuda", dtype=torch.int32)
    out = K.attn_fused(q, k, v, valid_len=vl)
    ref = _attn_ref(q.cpu(), k.cpu(), v.cpu(), valid=vl.cpu())
    _assert_close(out, ref, atol=3e-2, what="attn_fused masked")


def test_attn_fused_causal_and_gqa():
    B, nh, nhk, S, D = 2, 8, 2, 130, 96
    q = torch.randn(B, nh, S, D, device="cuda").bfloat16()
    k = torch.randn(B, nhk, S, D, device="cuda").bfloat16()
    v = torch.randn(B, nhk, S, D, device="cuda").bfloat16()
    out = K.attn_fused(q, k, v, causal=True)
    ref = _attn_ref(q.cpu(), k.cpu(), v.cpu(), causal=True)
    _assert_close(out, ref, atol=3e-2, what="attn_fused causal gqa")


def test_attn_fused_strided_views():
    """Q/K/V as strided views of a fused qkv buffer (the model path)."""
    B, S, nh, D = 2, 33, 4, 32
    qkv = torch.randn(B, S, 3, nh, D, device="cuda").bfloat16()
    qv = qkv[:, :, 0].permute(0, 2, 1, 3)
    kv = qkv[:, :, 1].permute(0, 2, 1, 3)
    vv = qkv[:, :, 2].permute(0, 2, 1, 3)
    out = K.attn_fused(qv, kv, vv)
    ref = _attn_ref(qv.contiguous().cpu(), kv.contiguous().cpu(),
                    vv.contiguous().cpu())
    _assert_close(out, ref, atol=3e-2, what="attn_fused strided")


def test_attn_fused_long_seq_causal():
    B, nh, S, D = 1, 2, 555, 128
    q = torch.randn(B, nh, S, D, device="cuda").bfloat16()
    k = torch.randn(B, nh, S, D, device="cuda").bfloat16()
    v = torch.randn(B, nh, S, D, device="cuda").bfloat16()
    out = K.attn_fused(q, k, v, causal=True)
    ref = _attn_ref(q.cpu(), k.cpu(), v.cpu(), causal=True)
    _assert_close(out, ref, atol=3e-2, what="attn_fused long causal")


# ---------------------------------------------------------- reshape ops

def test_qkv_split_no_rope():
    B, S, nh, nkv, d = 2, 5, 3, 3, 32
    qkv = torch.randn(B * S, (nh + 2 * nkv) * d, device="cuda").bfloat16()
    q, k, vt = K.qkv_split(qkv, B, S, nh, nkv, d)
    ref = qkv.view(B, S, nh + 2 * nkv, d).float()
    rq = ref[:, :, :nh].permute(0, 2, 1, 3).reshape(B * nh, S, d)
    rk = ref[:, :, nh:nh + nkv].permute(0, 2, 1, 3).reshape(B * nkv, S, d)
    rv = ref[:, :, nh + nkv:].permute(0, 2, 1, 3).reshape(B * nkv, S, d)
    assert torch.equal(q.float().cpu(), rq.cpu())
    assert torch.equal(k.float().cpu(), rk.cpu())
    assert torch.equal(vt.float().cpu(), rv.transpose(1, 2).contiguous().cpu())


def test_qkv_split_with_rope():
    B, S, nh, nkv, d = 1, 4, 2, 2, 64
    qkv = torch.randn(B * S, (nh + 2 * nkv) * d, device="cuda").bfloat16()
    inv = 1.0 / (10000 ** (torch.arange(d // 2).float() * 2 / d))
    ang = torch.outer(torch.arange(16).float(), inv)
    cos_t, sin_t = ang.cos().cuda(), ang.sin().cuda()
    pos = torch.arange(S, dtype=torch.int32, device="cuda").repeat(B)
    q, k, vt = K.qkv_split(qkv, B, S, nh, nkv, d, cos_t, sin_t, pos)
    # reference: split then rope rows
    ref = qkv.view(B * S, nh + 2 * nkv, d).clone().cpu()
    qk_ref = R.rope(ref[:, :nh + nkv].contiguous(), cos_t.cpu(),
                    sin_t.cpu(), pos.cpu())
    rq = qk_ref[:, :nh].view(B, S, nh, d).permute(0, 2, 1, 3)\
        .reshape(B * nh, S, d)
    _assert_close(q, rq, atol=1e-2, what="qkv_split rope q")
    rv = ref[:, nh + nkv:].float().view(B, S, nkv, d)\
        .permute(0, 2, 3, 1).reshape(B * nkv, d, S)
    assert torch.equal(vt.float().cpu(), rv.cpu())


def test_merge_heads_roundtrip():
    B, S, nh, d = 2, 7, 4, 32
    ctx = torch.randn(B * nh, S, d, device="cuda").bfloat16()
    out = K.merge_heads(ctx, B, S, nh, d)
    ref = ctx.view(B, nh, S, d).permute(0, 2, 1, 3).reshape(B * S, nh * d)
    assert torch.equal(out.cpu(), ref.cpu())


def test_silu_mul_fused():
    gu = torch.randn(6, 128, device="cuda").bfloat16()
    out = K.silu_mul_fused(gu, 64)
    ref = R.silu_mul(gu[:, :64].cpu(), gu[:, 64:].cpu())
    _assert_close(out, ref, what="silu_mul_fused")


# ----------------------------------------------------------- attn decode

def test_attn_decode_parity():
    B, H, Hkv, Smax, D = 2, 8, 4, 256, 96
    q = torch.randn(B, H, D, device="cuda").bfloat16()
    kc = torch.randn(B, Hkv, Smax, D, device="cuda").bfloat16()
    vc = torch.randn(B, Hkv, Smax, D, device="cuda").bfloat16()
    lens = torch.tensor([100, 256], device="cuda", dtype=torch.int32)
    out = K.attn_decode(q, kc, vc, lens, scale=D ** -0.5)
    ref = R.attn_decode(q.cpu(), kc.cpu(), vc.cpu(), lens.cpu(), D ** -0.5)
    _assert_close(out, ref, atol=2e-2, what="attn decode")


def test_kv_append():
    B, Hkv, Smax, D = 2, 4, 64, 96
    kc = torch.zeros(B, Hkv, Smax, D, device="cuda").bfloat16()
    vc = torch.zeros(B, Hkv, Smax, D, device="cuda").bfloat16()
    kn = torch.randn(B, Hkv, D, device="cuda").bfloat16()
    vn = torch.randn(B, Hkv, D, device="cuda").bfloat16()
    pos = torch.tensor([3, 10], device="cuda", dtype=torch.int32)
    K.kv_append(kn, vn, kc, vc, pos)
    torch.cuda.synchronize()
    assert torch.equal(kc[0, :, 3], kn[0])
    assert torch.equal(vc[1, :, 10], vn[1])
    assert kc[0, :, 4].abs().sum() == 0


@pytest.mark.parametrize("G,M,N,Kd,bias_gelu,out_f32", [
    # full tiles only (16x14 = 224): bf16 staged epilogue, two K-steps
    (1, 4096, 3584, 128, True, False),
    # one K-step: every prefetch past it is clamped
    (1, 4096, 3584, 64, False, False),
    # 17x14 tiles with partial last row/column tiles: guarded scalar
    # epilogue, odd K-step count; bf16 then f32 output
    (1, 4097, 3330, 192, True, False),
    (1, 4097, 3330, 192, True, True),
    # batched over a shared 2-D B (strideB == 0): 16x2x7 = 224 tiles
    (7, 4096, 512, 128, False, False),
])
def test_gemm8_large_shapes(G, M, N, Kd, bias_gelu, out_f32):
    """Shapes with >= 224 tiles of 256x256 run the deep-pipelined kernel."""
    assert K.gemm_route(M, N, Kd, G) == "gemm8"
    a = torch.randn(*((G,) if G > 1 else ()), M, Kd, device="cuda").bfloat16()
    b = torch.randn(N, Kd, device="cuda").bfloat16()
    bias = torch.randn(N, device="cuda") if bias_gelu else None
    act = "gelu" if bias_gelu else "none"
    out = K.gemm_nt(a, b, bias=bias, act=act, out_f32=out_f32)
    assert out.dtype == (torch.float32 if out_f32 else torch.bfloat16)
    ref = R.gemm_nt(a.cpu(), b.cpu(),
                    bias.cpu() if bias_gelu else None, act=act)
    _assert_close(out, ref, rtol=3e-2, atol=Kd ** 0.5 * 2e-2,
                  what=f"gemm8 {G}x{M}x{N}x{Kd}")


def test_gemm8_transpose_check():
    M, N, Kd = 4096, 3584, 64
    assert K.gemm_route(M, N, Kd, 1) == "gemm8"
    a = torch.eye(M, Kd, device="cuda").bfloat16()
    b = (torch.arange(N * Kd, device="cuda").reshape(N, Kd).bfloat16()
         / (N * Kd))
    out = K.gemm_nt(a, b)
    ref = R.gemm_nt(a.cpu(), b.cpu())
    _assert_close(out, ref, what="gemm8 transpose check")


def test_gemm8_n_chunked(monkeypatch):
    """INFOMESH_GEMM8_CHUNK=1 splits a B panel above 3 MB into column
    chunks (here 1536 + 1536 + 512 of N=3584), each launched with its
    own B, bias and C offset and the full row stride. Every element sees
    the same K order as in the single launch, so the two are bit-equal."""
    M, N, Kd = 4096, 3584, 768
    assert K.gemm_route(M, N, Kd, 1) == "gemm8"
    a = torch.randn(M, Kd, device="cuda").bfloat16()
    b = torch.randn(N, Kd, device="cuda").bfloat16()
    bias = torch.randn(N, device="cuda")
    monkeypatch.delenv("INFOMESH_GEMM8_CHUNK", raising=False)
    whole = K.gemm_nt(a, b, bias=bias)
    monkeypatch.setenv("INFOMESH_GEMM8_CHUNK", "1")
    chunked = K.gemm_nt(a, b, bias=bias)
    torch.cuda.synchronize()
    ref = R.gemm_nt(a.cpu(), b.cpu(), bias.cpu())
    _assert_close(chunked, ref, rtol=3e-2, atol=Kd ** 0.5 * 2e-2,
                  what="gemm8 chunked")
    assert torch.equal(chunked, whole)


def test_topk_constant_scores_valid():
    """Constant scores: every element ties the threshold. The
    tie-tolerant compact keeps a capped set of interchangeable
    candidates, so the result is a VALID top-k (it used to be a loud
    overflow error)."""
    from infomesh_amd.ops.kernels import TopK
    scores = torch.ones(1, 300_000, device="cuda")
    t = TopK("cuda")
    v, i = t(scores, 10)
    assert (v == 1.0).all() and len(set(i[0].tolist())) == 10


def test_topk_producer_histogram_matches_own_pass1():
    """ext_hist1 (the producer-fused pass 1) against the selector's own
    hist1 pass. N = 20 011 is no multiple of 4 (scalar tails run) and
    spans two grid chunks of 16 384; exact zeros and a negative block
    exercise both branches of the ordered-float mapping. The 100th
    value is untied here, so no tie is dropped and indices are
    deterministic."""
    from infomesh_amd.ops.kernels import TopK
    g = torch.Generator().manual_seed(7)
    host = torch.randn(3, 20_011, generator=g)
    host[:, 5::97] = 0.0
    host[:, 12_000:13_000] = -host[:, 12_000:13_000].abs() - 1.0
    # float_to_ordered (common.h): negative -> ~bits, else bits | sign
    bits = host.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    ordered = torch.where(bits >= 0x80000000, bits ^ 0xFFFFFFFF,
                          bits | 0x80000000)
    top = ordered >> 24
    hist = torch.stack([torch.bincount(r, minlength=256) for r in top])
    assert hist.shape == (3, 256) and int(hist.sum()) == host.numel()
    scores = host.cuda()
    v_ext, i_ext = TopK()(scores, 100,
                          ext_hist1=hist.to(torch.int32).cuda())
    v_own, i_own = TopK()(scores, 100)
    assert torch.equal(v_ext, v_own) and torch.equal(i_ext, i_own)
    rv, _ = torch.topk(scores, 100, dim=-1)
    assert torch.equal(v_own, rv)


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,Kd", [(128, 131072, 384), (100, 70000, 384),
                                    (128, 131072 + 100, 128)])
def test_dense_scores_streaming(M, N, Kd):
    """The streaming dense-score kernel (densescore.hip, explicit
    opt-in) — parity vs the fp32 oracle, incl. N tails and
    non-multiple-of-16 M."""
    torch.manual_seed(5)
    a = torch.randn(M, Kd, device="cuda").bfloat16()
    b = torch.randn(N, Kd, device="cuda").bfloat16()
    out = K.dense_scores(a, b)
    assert out is not None and out.dtype == torch.float32
    ref = a.float() @ b.float().T
    _assert_close(out, ref, rtol=3e-2, atol=Kd ** 0.5 * 2e-2,
                  what=f"dense_scores {M}x{N}x{Kd}")


@pytest.mark.gpu
def test_dense_scores_matches_generic_tile():
    """Same shape through the streaming kernel and the generic tile path
    (same MFMA order, f32 accum) must agree bitwise."""
    torch.manual_seed(6)
    a = torch.randn(64, 384, device="cuda").bfloat16()
    b = torch.randn(70000, 384, device="cuda").bfloat16()
    stream = K.dense_scores(a, b)
    assert stream is not None
    generic = K.gemm_nt(a, b, out_f32=True)
    torch.cuda.synchronize()
    assert torch.equal(stream, generic)


def test_topk_massively_tied_scores():
    """Degenerate planes (tiny-vocab corpora) produce tens of thousands
    of EXACTLY tied scores; the selector must return a valid top-k
    (correct values; tie membership arbitrary) instead of overflowing
    (round-2 regression: serving 500s on tied corpora)."""
    g = torch.Generator(device="cuda").manual_seed(0)
    B, N, k = 8, 200_000, 100
    # three tied levels: 5.0 (50k), 3.0 (100k), 1.0 (rest)
    scores = torch.ones(B, N, device="cuda")
    scores[:, :50_000] = 5.0
    scores[:, 50_000:150_000] = 3.0
    perm = torch.randperm(N, generator=g, device="cuda")
    scores = scores[:, perm].contiguous()
    vals, idx = K.topk(scores, k)
    assert (vals == 5.0).all(), "all top-100 must come from the 5.0 tier"
    assert (scores[0, idx[0].long()] == 5.0).all()
    assert len(set(idx[0].tolist())) == k, "indices must be distinct"
    # threshold tier bigger than the whole candidate region, k spanning
    scores2 = torch.full((2, N), 2.0, device="cuda")
    scores2[:, :10] = 7.0
    vals2, idx2 = K.topk(scores2, 50)
    assert (vals2[:, :10] == 7.0).all() and (vals2[:, 10:] == 2.0).all()
    assert len(set(idx2[0].tolist())) == 50


def test_dense_scores_fp8_parity_and_retrieval():
    """FP8 (e4m3) dense plane: scores within quantization tolerance of
    the fp32 oracle, and self-retrieval (query == doc) still wins."""
    import numpy as np
    torch.manual_seed(11)
    M, N, D = 96, 70_000, 384
    b = torch.nn.functional.normalize(
        torch.randn(N, D, device="cuda"), dim=-1)
    a = b[:M].clone()                      # queries = first M docs
    a8 = a.to(torch.float8_e4m3fn)
    b8 = b.to(torch.float8_e4m3fn)
    out = K.dense_scores_fp8(a8.contiguous(), b8.contiguous())
    assert out is not None
    ref = a8.float() @ b8.float().T        # exact product of quantized
    _assert_close(out, ref, rtol=1e-3, atol=1e-3, what="fp8 exact")
    full = a @ b.T                         # unquantized oracle
    err = (out - full).abs().max().item()
    assert err < 0.06, f"fp8 quantization error too large: {err}"
    top1 = out.argmax(dim=1)
    agree = (top1 == torch.arange(M, device="cuda")).float().mean()
    assert agree > 0.95, f"self-retrieval {agree}"


def test_gpu_shard_fp8_mode():
    """End-to-end shard in fp8 embedding mode: hybrid search works and
    dense self-retrieval holds."""
    import numpy as np
    from infomesh_amd.index.synth import build_synth_shard
    shard = build_synth_shard(50_000, avg_len=60, device="cuda",
                              seed=5, emb_dtype="fp8")
    assert shard.embeddings.dtype == torch.float8_e4m3fn
    q = shard.embeddings[:8].float()       # queries = docs 0..7
    terms = [np.array([3, 5]) for _ in range(8)]
    hits = shard.search(terms, q, k=10)
    top = hits.dense_ids[:, 0].cpu()
    gids = shard.global_ids[:8].cpu()
    assert (top == gids).float().mean() > 0.8
    # HBM halves vs bf16 for the embedding plane
    bytes_fp8 = shard.embeddings.numel() * shard.embeddings.element_size()
    assert bytes_fp8 == 50_000 * 384
