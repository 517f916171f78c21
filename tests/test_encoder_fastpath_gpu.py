"""The encoder's fast path against the plain kernel sequence, bit for bit.

Every item of the fast path (attention writing the merged layout, the
short attention tile, the CLS-only tail of the last layer, the one-kernel
embedding front) only drops work the result does not need, so every
comparison here is torch.equal against the present kernels in the same
process, never a tolerance.
"""
from __future__ import annotations

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from infomesh_amd.ops import _build
    _build.build()

from infomesh_amd.models.bert import (BertConfig, BertEncoder,
                                      cls_tail_same_kernel,
                                      init_bert_weights)
from infomesh_amd.models.encoder import BGE_SMALL, EmbeddingEncoder
from infomesh_amd.ops import kernels as K


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.manual_seed(0)


TINY_BERT = BertConfig(vocab_size=2048, hidden=128, layers=2, heads=4,
                       ffn=256, max_pos=64)


def _rand(*shape):
    return torch.randn(*shape, device="cuda").bfloat16()


def _i32(vals):
    return torch.tensor(vals, dtype=torch.int32, device="cuda")


# ------------------------------------------------------------ output view

SENTINEL = -1.5      # exact in bf16


def _merged_out(B, S, nh, D, pad=16):
    """An over-allocated buffer of SENTINEL and, inside it, the head view
    [B, nh, S, D] of a merged [B*S, nh*D] block."""
    buf = torch.full((pad + B * S * nh * D + pad,), SENTINEL,
                     device="cuda", dtype=torch.bfloat16)
    merged = buf[pad:pad + B * S * nh * D].view(B * S, nh * D)
    return buf, merged, merged.view(B, S, nh, D).permute(0, 2, 1, 3)


def _check_out_view(q, k, v, vl):
    B, nh, S, D = q.shape
    ref = K.merge_heads(K.attn_fused(q, k, v, valid_len=vl), B, S, nh, D)
    buf, merged, view = _merged_out(B, S, nh, D)
    ret = K.attn_fused(q, k, v, valid_len=vl, out=view)
    assert ret is view
    assert torch.equal(merged, ref)
    assert (buf[:16] == SENTINEL).all() and (buf[-16:] == SENTINEL).all()


@pytest.mark.parametrize("D", [32, 64])
@pytest.mark.parametrize("S", [1, 17, 32, 33, 64, 100])
def test_out_view_matches_merge_heads(D, S):
    B, nh = 3, 4
    q, k, v = (_rand(B, nh, S, D) for _ in range(3))
    _check_out_view(q, k, v, _i32([S, 1, 0]))
    _check_out_view(q, k, v, None)


def test_out_view_gqa():
    B, nh, nhk, S, D = 3, 4, 2, 33, 32
    q = _rand(B, nh, S, D)
    k, v = _rand(B, nhk, S, D), _rand(B, nhk, S, D)
    _check_out_view(q, k, v, _i32([33, 7, 0]))


def test_out_view_packed_qkv_and_padded_rows():
    """Q/K/V as strided views of one packed QKV buffer; the out view's
    rows lie in a wider buffer whose other columns keep the sentinel."""
    B, S, nh, D = 3, 17, 4, 32
    qkv = _rand(B, S, 3, nh, D)
    q, k, v = (qkv[:, :, j].permute(0, 2, 1, 3) for j in range(3))
    vl = _i32([17, 1, 0])
    _check_out_view(q, k, v, vl)
    ref = K.merge_heads(K.attn_fused(q, k, v, valid_len=vl), B, S, nh, D)
    wide = torch.full((B * S, nh * D + 64), SENTINEL, device="cuda",
                      dtype=torch.bfloat16)
    view = wide[:, 32:32 + nh * D].unflatten(0, (B, S)) \
        .unflatten(2, (nh, D)).permute(0, 2, 1, 3)
    K.attn_fused(q, k, v, valid_len=vl, out=view)
    assert torch.equal(wide[:, 32:32 + nh * D], ref)
    assert (wide[:, :32] == SENTINEL).all()
    assert (wide[:, 32 + nh * D:] == SENTINEL).all()


# ---------------------------------------------------------- short variant

def _both_variants(q, k, v, **kw):
    gen = K.attn_fused(q, k, v, variant=1, **kw)
    short = K.attn_fused(q, k, v, variant=2, **kw)
    assert short is not None, "variant 2 refused an eligible shape"
    assert torch.equal(short, gen)
    assert torch.equal(K.attn_fused(q, k, v, variant=0, **kw), gen)


@pytest.mark.parametrize("D", [32, 64, 96, 128])
@pytest.mark.parametrize("S", [1, 15, 16, 17, 31, 32])
def test_short_variant_square(D, S):
    B, nh = 3, 4
    q, k, v = (_rand(B, nh, S, D) for _ in range(3))
    _both_variants(q, k, v)
    _both_variants(q, k, v, valid_len=_i32([0, 1, S]))


@pytest.mark.parametrize("D", [32, 64, 96, 128])
def test_short_variant_tail_shape(D):
    """Sq = 1 against Sk = 32: the CLS-only tail."""
    B, nh = 3, 4
    q, k, v = _rand(B, nh, 1, D), _rand(B, nh, 32, D), _rand(B, nh, 32, D)
    _both_variants(q, k, v, valid_len=_i32([0, 1, 32]))
    _both_variants(q, k, v)


@pytest.mark.parametrize("D", [32, 64, 96, 128])
def test_short_variant_causal(D):
    B, nh = 3, 4
    q, k, v = (_rand(B, nh, 32, D) for _ in range(3))
    _both_variants(q, k, v, causal=True)
    _both_variants(q, k, v, causal=True, valid_len=_i32([0, 1, 32]))


@pytest.mark.parametrize("D", [32, 64, 96, 128])
def test_short_variant_causal_gqa_rect(D):
    B, nh, nhk = 3, 4, 2
    q = _rand(B, nh, 8, D)
    k, v = _rand(B, nhk, 32, D), _rand(B, nhk, 32, D)
    _both_variants(q, k, v, causal=True)


def test_short_variant_refused_past_its_tile():
    B, nh, D = 2, 2, 32
    q32, q33 = _rand(B, nh, 32, D), _rand(B, nh, 33, D)
    k32, k33 = _rand(B, nh, 32, D), _rand(B, nh, 33, D)
    assert K.attn_fused(q32, k33, k33, variant=2) is None
    assert K.attn_fused(q33, k32, k32, variant=2) is None
    assert K.attn_fused(q33, k33, k33, variant=2) is None


@pytest.mark.parametrize("Sq,Sk", [(32, 32), (33, 33), (32, 33), (33, 32)])
def test_variant_choice_across_the_border(Sq, Sk):
    B, nh, D = 3, 4, 64
    q, k, v = _rand(B, nh, Sq, D), _rand(B, nh, Sk, D), _rand(B, nh, Sk, D)
    vl = _i32([Sk, 1, 0])
    assert torch.equal(K.attn_fused(q, k, v, valid_len=vl, variant=0),
                       K.attn_fused(q, k, v, valid_len=vl, variant=1))


# -------------------------------------------------------- embedding front

@pytest.mark.parametrize("H", [128, 384])
@pytest.mark.parametrize("S", [32, 64])
def test_embed_layernorm_matches_composition(H, S):
    B, V = 3, 1000
    word, pos = _rand(V, H), _rand(S + 5, H)
    gamma, beta = _rand(H), _rand(H)
    ids = torch.randint(0, V, (B, S), dtype=torch.int32, device="cuda")
    ids[0, 0], ids[0, 1], ids[2, S - 1] = 0, V - 1, V - 1
    ids[1, S // 2:] = 0                        # pad id
    flat = ids.reshape(-1)
    pos_ids = torch.arange(S, device="cuda", dtype=torch.int32).repeat(B)
    ref = K.layernorm(K.add(K.gather(word, flat), K.gather(pos, pos_ids)),
                      gamma, beta, eps=1e-12)
    out = K.embed_layernorm(word, pos, flat, S, gamma, beta, eps=1e-12)
    assert torch.equal(out, ref)


def test_layernorm_strided_residual():
    """The tail's LN1: residual rows S*H apart give the bits of the same
    rows packed."""
    B, S, H = 5, 32, 128
    x, full = _rand(B, H), _rand(B * S, H)
    gamma, beta = _rand(H), _rand(H)
    res = full.view(B, S, H)[:, 0]
    assert not res.is_contiguous()
    assert torch.equal(K.layernorm(x, gamma, beta, residual=res),
                       K.layernorm(x, gamma, beta,
                                   residual=res.contiguous()))


# --------------------------------------------------------------- CLS tail

def _tiny_pair():
    w = init_bert_weights(TINY_BERT, 7, "cuda")
    return (BertEncoder(TINY_BERT, w, fast_path=False),
            BertEncoder(TINY_BERT, w))


def _ragged(B, S, vocab):
    ids = torch.randint(4, vocab, (B, S), dtype=torch.int32, device="cuda")
    lens = torch.randint(1, S + 1, (B,), dtype=torch.int32, device="cuda")
    lens[0], lens[1] = S, 1
    ids[torch.arange(S, device="cuda")[None, :] >= lens[:, None]] = 0
    return ids, lens


@pytest.mark.parametrize("S", [32, 17])
def test_cls_tail_taken(S):
    plain, fast = _tiny_pair()
    B, H, F = 66, TINY_BERT.hidden, TINY_BERT.ffn
    for N, Kd in ((H, H), (F, H), (H, F)):
        # both row counts on the pipelined 64x64 tile
        assert K.gemm_tile(B, N, Kd, 1) == (64, 64, 64, True)
        assert K.gemm_tile(B * 32, N, Kd, 1) == (64, 64, 64, True)
    assert cls_tail_same_kernel(B, B * 32, H, F)
    ids, lens = _ragged(B, S, TINY_BERT.vocab_size)
    ref = plain.forward(ids, lens)[:, :1]
    out = fast.forward(ids, lens, cls_only=True)
    assert out.shape == (B, 1, H) and out.is_contiguous()
    assert torch.equal(out, ref)
    assert torch.equal(fast.forward(ids, lens), plain.forward(ids, lens))


def test_cls_tail_not_taken_at_small_batch():
    plain, fast = _tiny_pair()
    B, S, H, F = 3, 32, TINY_BERT.hidden, TINY_BERT.ffn
    assert not cls_tail_same_kernel(B, B * S, H, F)      # gemv at M = 3
    assert not cls_tail_same_kernel(64, 64 * S, H, F)    # 64x128 tile
    ids, lens = _ragged(B, S, TINY_BERT.vocab_size)
    out = fast.forward(ids, lens, cls_only=True)
    assert out.shape == (B, 1, H)
    assert out.stride(0) == S * H                # a view of the full layer
    assert torch.equal(out, plain.forward(ids, lens)[:, :1])
    # CLS pooling reads the strided rows in place
    assert torch.equal(K.pool(out, lens, mode="cls"),
                       K.pool(plain.forward(ids, lens), lens, mode="cls"))


# ---------------------------------------------------------- whole encoder

@pytest.fixture(scope="module")
def bge_plain_embeddings():
    """Two seeded id batches as in the benchmark and their embeddings on
    the plain path (eager), computed once."""
    enc = EmbeddingEncoder(device="cuda", cfg=BGE_SMALL, use_graph=False,
                           fast_path=False)
    batches = []
    for seed in (0, 13):
        g = torch.Generator().manual_seed(seed)
        ids = torch.randint(4, 30522, (128, 32), generator=g,
                            dtype=torch.int32)
        ids[:, 0] = 1
        ids = ids.cuda()
        lens = torch.full((128,), 32, dtype=torch.int32, device="cuda")
        batches.append((ids, lens, enc.encode_ids(ids, lens).clone()))
    return batches


@pytest.mark.parametrize("use_graph", [True, False])
def test_whole_encoder_bit_identical(bge_plain_embeddings, use_graph):
    H, F = BGE_SMALL.hidden, BGE_SMALL.ffn
    assert cls_tail_same_kernel(128, 128 * 32, H, F)
    fast = EmbeddingEncoder(device="cuda", cfg=BGE_SMALL,
                            use_graph=use_graph)
    # two consecutive calls with different ids: on the graph these go
    # through the same static buffers
    for ids, lens, ref in bge_plain_embeddings:
        assert torch.equal(fast.encode_ids(ids, lens), ref)
    if use_graph:
        plain = EmbeddingEncoder(device="cuda", cfg=BGE_SMALL,
                                 fast_path=False)
        for ids, lens, ref in bge_plain_embeddings:
            assert torch.equal(plain.encode_ids(ids, lens), ref)
