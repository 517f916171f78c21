"""Typed torch-tensor wrappers over the HIP extension.

Every function validates layout/dtype, then launches the hand-written
CDNA4 kernel on the current HIP stream. No eager-PyTorch fallback on
GPU — a missing extension raises GPU001 (errors.GpuExtensionMissing).
"""
from __future__ import annotations

import torch

from . import _ext

ACT = {"none": 0, "gelu": 1, "silu": 2, "relu": 3, "tanh": 4}


def _ptr(t: torch.Tensor | None) -> int | None:
    return None if t is None else t.data_ptr()


def _check(t: torch.Tensor, dtype: torch.dtype, name: str) -> None:
    assert t.is_cuda, f"{name} must be on GPU"
    assert t.dtype == dtype, f"{name} must be {dtype}, got {t.dtype}"
    assert t.is_contiguous(), f"{name} must be contiguous"


def gemm_route(M: int, N: int, K: int, G: int) -> str:
    """Which kernel family gemm_nt runs a [G,M,K] x [N,K] product on."""
    if M <= 16:
        # skinny-M decode path: wave-per-column GEMV (csrc/gemv.hip)
        return "gemv"
    if (M >= 4096 and N >= 512 and K % 64 == 0
            and ((M + 255) // 256) * ((N + 255) // 256) * max(G, 1) >= 224):
        # big projection shapes: deep-pipelined 256x256 tile (gemm8.hip)
        # (tile count must fill the chip at 1 block/CU)
        return "gemm8"
    return "gemm"


# route -> C entry point; the three share one signature
_GEMM_ENTRY = {"gemv": "infomesh_gemv_bf16_nt",
               "gemm8": "infomesh_gemm8_bf16_nt",
               "gemm": "infomesh_gemm_bf16_nt"}


def gemm_tile(M: int, N: int, K: int, G: int) -> tuple[int, int, int, bool]:
    """(bm, bn, bk, pipelined) of the gemm.hip tile for this shape."""
    code = _ext.lib().infomesh_gemm_tile(M, N, K, G)
    return code & 0xff, code >> 8 & 0xff, code >> 16 & 0xff, bool(code >> 24)


def gemm_nt(a: torch.Tensor, b: torch.Tensor,
            bias: torch.Tensor | None = None,
            act: str = "none", alpha: float = 1.0,
            out_f32: bool = False,
            out: torch.Tensor | None = None) -> torch.Tensor:
    """C[...,M,N] = act(alpha * A[...,M,K] @ B[...,N,K]^T + bias[N]).

    A: [M,K] or [G,M,K] bf16; B: [N,K] or [G,N,K] bf16 (shared across the
    batch when 2-D). bias: [N] f32 or None."""
    sq_a = a.dim() == 2
    if sq_a:
        a = a.unsqueeze(0)
    if b.dim() == 2:
        b = b.unsqueeze(0).expand(a.shape[0], *b.shape)
    G, M, K = a.shape
    Gb, N, Kb = b.shape
    assert K == Kb and Gb == G, f"shape mismatch {a.shape} x {b.shape}"
    assert K % 32 == 0, f"K={K} must be a multiple of 32"
    _check(a, torch.bfloat16, "A")
    assert b.dtype == torch.bfloat16
    strideB = 0 if (G > 1 and b.stride(0) == 0) else N * K
    if strideB != 0:
        assert b.is_contiguous()
    else:
        assert b[0].is_contiguous()
    if bias is not None:
        _check(bias, torch.float32, "bias")
        assert bias.numel() == N
    dtype = torch.float32 if out_f32 else torch.bfloat16
    if out is None:
        out = torch.empty((G, M, N), device=a.device, dtype=dtype)
    else:
        assert out.shape == (G, M, N) and out.dtype == dtype and out.is_contiguous()
    fn = getattr(_ext.lib(), _GEMM_ENTRY[gemm_route(M, N, K, G)])
    fn(a.data_ptr(), b.data_ptr(), out.data_ptr(), _ptr(bias),
       M, N, K, G, M * K, strideB, M * N,
       ACT[act], alpha, int(out_f32), _ext.stream_ptr())
    return out.squeeze(0) if sq_a else out


def gemm_bmax_width(M: int, N: int, K: int, G: int = 1) -> int:
    """Columns per block maximum of gemm_nt_bmax at this shape (the
    extension reports it: 64, or 32 at M <= 64), 0 when the shape is
    not covered (the gemv and gemm8 routes)."""
    if gemm_route(M, N, K, G) != "gemm":
        return 0
    return _ext.lib().infomesh_gemm_bmax_width(M, N, K, G)


def gemm_nt_bmax(a: torch.Tensor, b: torch.Tensor, alpha: float = 1.0,
                 out: torch.Tensor | None = None,
                 bmax: torch.Tensor | None = None
                 ) -> tuple[torch.Tensor, torch.Tensor, int] | None:
    """gemm_nt(a [M,K], b [N,K], out_f32=True) that also returns the
    block maxima of every score row: (scores [M,N] f32 — the bits
    gemm_nt writes —, bmax [M, ceil(N/W)] f32, W), bmax[m, j] =
    max(scores[m, j*W:(j+1)*W]) in the selector's order (-0.0 < +0.0).
    None, with nothing launched, when gemm_bmax_width is 0."""
    M, K = a.shape
    N, Kb = b.shape
    assert K == Kb and K % 32 == 0, f"shape mismatch {a.shape} x {b.shape}"
    _check(a, torch.bfloat16, "A")
    _check(b, torch.bfloat16, "B")
    W = gemm_bmax_width(M, N, K)
    if W == 0:
        return None
    NB = (N + W - 1) // W
    if out is None:
        out = torch.empty((M, N), device=a.device, dtype=torch.float32)
    if bmax is None:
        bmax = torch.empty((M, NB), device=a.device, dtype=torch.float32)
    for t, shape, name in ((out, (M, N), "out"), (bmax, (M, NB), "bmax")):
        _check(t, torch.float32, name)
        assert t.shape == shape, f"{name} must be {shape}, got {t.shape}"
    rc = _ext.lib().infomesh_gemm_bf16_nt_bmax(
        a.data_ptr(), b.data_ptr(), out.data_ptr(), None, bmax.data_ptr(),
        M, N, K, 1, M * K, N * K, M * N, ACT["none"], alpha,
        _ext.stream_ptr())
    assert rc == 0, "tile changed between gemm_bmax_width and the launch"
    return out, bmax, W


def dense_scores(a: torch.Tensor, b: torch.Tensor, alpha: float = 1.0,
                 out: torch.Tensor | None = None) -> torch.Tensor | None:
    """Streaming dense-score GEMM (densescore.hip): C[M,N] f32 =
    alpha * A[M,K]bf16 @ B[N,K]^T for M<=128, K%128==0, huge N — the
    whole query block in LDS, docs streamed HBM->registers.

    Measured on MI355X at 128 x 1.25M x 384: 529 us vs 511 us for the
    generic 128^2 tile (both ~3.1 TB/s effective against a ~5.4 TB/s
    practical mixed-stream ceiling), so gemm_nt does NOT auto-dispatch
    here; this stays an explicit opt-in and a tuning baseline.
    Returns None when the shape is ineligible."""
    M, K = a.shape
    N = b.shape[0]
    _check(a, torch.bfloat16, "A")
    _check(b, torch.bfloat16, "B")
    if out is None:
        out = torch.empty(M, N, device=a.device, dtype=torch.float32)
    rc = _ext.lib().infomesh_dense_scores(
        a.data_ptr(), b.data_ptr(), out.data_ptr(), M, N, K, alpha,
        _ext.stream_ptr())
    return out if rc == 0 else None


def dense_scores_fp8(a: torch.Tensor, b: torch.Tensor,
                     alpha: float = 1.0,
                     out: torch.Tensor | None = None
                     ) -> torch.Tensor | None:
    """FP8 (OCP e4m3) streaming dense-score GEMM (densescore8.hip):
    C[M,N] f32 = A[M,K] @ B[N,K]^T with fp8 operands — half the read
    traffic and half the HBM footprint of the bf16 plane (the plane is
    bandwidth-bound; non-scaled fp8 MFMA matches the bf16 rate). Both
    operands must be torch.float8_e4m3fn. Returns None when the shape
    is ineligible."""
    M, K = a.shape
    N = b.shape[0]
    assert a.dtype == torch.float8_e4m3fn and a.is_cuda and a.is_contiguous()
    assert b.dtype == torch.float8_e4m3fn and b.is_contiguous()
    if out is None:
        out = torch.empty(M, N, device=a.device, dtype=torch.float32)
    rc = _ext.lib().infomesh_dense_scores_fp8(
        a.data_ptr(), b.data_ptr(), out.data_ptr(), M, N, K, alpha,
        _ext.stream_ptr())
    return out if rc == 0 else None


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
              residual: torch.Tensor | None = None, eps: float = 1e-12,
              return_residual: bool = False):
    """LayerNorm over the last dim; optionally fused residual add
    (y = LN(x + residual)); returns (y, x+residual) if requested.
    A 2-D residual may have any row stride that is a multiple of 8
    (rows of a larger buffer); its elements must be contiguous."""
    H = x.shape[-1]
    assert H % 8 == 0
    rows = x.numel() // H
    _check(x, torch.bfloat16, "x")
    out = torch.empty_like(x)
    res_out = None
    res_stride = H
    if residual is not None:
        assert residual.shape == x.shape
        assert residual.dtype == torch.bfloat16 and residual.is_cuda
        if not residual.is_contiguous():
            assert residual.dim() == 2 and residual.stride(1) == 1 \
                and residual.stride(0) >= H and residual.stride(0) % 8 == 0 \
                and residual.storage_offset() % 8 == 0, \
                "residual must be contiguous or a 2-D row-strided view"
            res_stride = residual.stride(0)
        if return_residual:
            res_out = torch.empty_like(x)
    _ext.lib().infomesh_layernorm(
        x.data_ptr(), _ptr(residual), out.data_ptr(), _ptr(res_out),
        gamma.data_ptr(), beta.data_ptr(), rows, H, eps, res_stride,
        _ext.stream_ptr())
    return (out, res_out) if return_residual else out


def embed_layernorm(word: torch.Tensor, pos: torch.Tensor,
                    ids: torch.Tensor, S: int, gamma: torch.Tensor,
                    beta: torch.Tensor, eps: float = 1e-12) -> torch.Tensor:
    """Embedding front in one kernel: out[r] = LN(bf16(word[ids[r]] +
    pos[r % S])) for ids [rows] i32 — the bits of gather, gather, add,
    layernorm. H <= 2048 (the wave-per-row norm kernel)."""
    _check(word, torch.bfloat16, "word")
    _check(pos, torch.bfloat16, "pos")
    _check(ids, torch.int32, "ids")
    _check(gamma, torch.bfloat16, "gamma")
    _check(beta, torch.bfloat16, "beta")
    H = word.shape[1]
    assert pos.shape[1] == H and gamma.numel() == H and beta.numel() == H
    assert 1 <= S <= pos.shape[0] and ids.numel() % S == 0
    out = torch.empty((ids.numel(), H), device=word.device,
                      dtype=torch.bfloat16)
    rc = _ext.lib().infomesh_embed_layernorm(
        word.data_ptr(), pos.data_ptr(), ids.data_ptr(), out.data_ptr(),
        gamma.data_ptr(), beta.data_ptr(), ids.numel(), S, H, eps,
        _ext.stream_ptr())
    assert rc == 0, f"embed_layernorm does not cover H={H}"
    return out


def rmsnorm(x: torch.Tensor, gamma: torch.Tensor,
            residual: torch.Tensor | None = None, eps: float = 1e-5,
            return_residual: bool = False):
    H = x.shape[-1]
    assert H % 8 == 0
    rows = x.numel() // H
    _check(x, torch.bfloat16, "x")
    out = torch.empty_like(x)
    res_out = None
    if residual is not None and return_residual:
        res_out = torch.empty_like(x)
    _ext.lib().infomesh_rmsnorm(
        x.data_ptr(), _ptr(residual), out.data_ptr(), _ptr(res_out),
        gamma.data_ptr(), rows, H, eps, _ext.stream_ptr())
    if return_residual:
        # with no residual input, the running residual IS the input
        return out, (res_out if res_out is not None else x)
    return out


def softmax(scores: torch.Tensor, scale: float = 1.0, causal: bool = False,
            valid_len: torch.Tensor | None = None,
            sq_dim: int | None = None) -> torch.Tensor:
    """Masked row softmax: f32 [G,Sq,Sk] -> bf16 [G,Sq,Sk]."""
    assert scores.dim() == 3
    _check(scores, torch.float32, "scores")
    G, Sq, Sk = scores.shape
    out = torch.empty_like(scores, dtype=torch.bfloat16)
    if valid_len is not None:
        _check(valid_len, torch.int32, "valid_len")
    _ext.lib().infomesh_softmax(
        scores.data_ptr(), out.data_ptr(), _ptr(valid_len),
        G, Sq, Sk, int(causal), scale, _ext.stream_ptr())
    return out


def bias_act(x: torch.Tensor, bias: torch.Tensor | None,
             act: str = "none") -> torch.Tensor:
    """In-place x = act(x + bias)."""
    N = x.shape[-1]
    assert N % 8 == 0
    _check(x, torch.bfloat16, "x")
    if bias is not None:
        _check(bias, torch.float32, "bias")
    _ext.lib().infomesh_bias_act(
        x.data_ptr(), _ptr(bias), x.numel() // N, N, ACT[act],
        _ext.stream_ptr())
    return x


def silu_mul(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    assert gate.shape == up.shape and gate.numel() % 8 == 0
    out = torch.empty_like(gate)
    _ext.lib().infomesh_silu_mul(gate.data_ptr(), up.data_ptr(),
                                 out.data_ptr(), gate.numel(),
                                 _ext.stream_ptr())
    return out


def add(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    assert a.shape == b.shape and a.numel() % 8 == 0
    out = torch.empty_like(a)
    _ext.lib().infomesh_add(a.data_ptr(), b.data_ptr(), out.data_ptr(),
                            a.numel(), _ext.stream_ptr())
    return out


def rope(x: torch.Tensor, cos_t: torch.Tensor, sin_t: torch.Tensor,
         pos: torch.Tensor, rot_dim: int | None = None) -> torch.Tensor:
    """In-place NeoX-style RoPE on x [rows, H, D] with pos [rows] i32 and
    host-precomputed cos/sin [max_pos, rot/2] f32 tables."""
    rows, H, D = x.shape
    rot = rot_dim or D
    _check(x, torch.bfloat16, "x")
    _check(pos, torch.int32, "pos")
    _ext.lib().infomesh_rope(
        x.data_ptr(), cos_t.data_ptr(), sin_t.data_ptr(), pos.data_ptr(),
        rows, H, D, rot, _ext.stream_ptr())
    return x


def gather(table: torch.Tensor, ids: torch.Tensor,
           scale: float = 1.0) -> torch.Tensor:
    """out[r] = table[ids[r]] * scale (embedding lookup)."""
    _check(table, torch.bfloat16, "table")
    _check(ids, torch.int32, "ids")
    H = table.shape[1]
    out = torch.empty((ids.numel(), H), device=table.device,
                      dtype=torch.bfloat16)
    _ext.lib().infomesh_gather(table.data_ptr(), ids.data_ptr(),
                               out.data_ptr(), ids.numel(), H, scale,
                               _ext.stream_ptr())
    return out


def pool(x: torch.Tensor, lens: torch.Tensor | None = None,
         mode: str = "cls", l2: bool = True) -> torch.Tensor:
    """[B,S,H] bf16 -> [B,H] f32 (CLS or masked-mean pooling, L2 option).
    CLS pooling also takes the CLS rows alone as a strided [B,1,H] view
    whose batch stride is a multiple of H."""
    B, S, H = x.shape
    if mode == "cls" and S == 1 and not x.is_contiguous():
        assert x.is_cuda and x.dtype == torch.bfloat16
        assert x.stride(2) == 1 and x.stride(0) % H == 0 and x.stride(0) > 0
        S = x.stride(0) // H      # the kernel reads row b*S of [B*S, H]
    else:
        _check(x, torch.bfloat16, "x")
    out = torch.empty((B, H), device=x.device, dtype=torch.float32)
    _ext.lib().infomesh_pool(
        x.data_ptr(), _ptr(lens), out.data_ptr(), B, S, H,
        {"cls": 0, "mean": 1}[mode], int(l2), _ext.stream_ptr())
    return out


def argmax(logits: torch.Tensor) -> torch.Tensor:
    rows, V = logits.shape
    _check(logits, torch.float32, "logits")
    out = torch.empty((rows,), device=logits.device, dtype=torch.int32)
    _ext.lib().infomesh_argmax(logits.data_ptr(), out.data_ptr(), rows, V,
                               _ext.stream_ptr())
    return out


class TopK:
    """Reusable top-k selector: keeps its workspace (histograms,
    counters and the candidate buffer, sized by the extension)
    allocated across calls, so a query plane pays no allocation per
    batch. Asynchronous like every other wrapper: launches on the
    current stream and returns without a host sync."""

    def __init__(self, device: torch.device | str = "cuda"):
        self.device = torch.device(device)
        self._ws: torch.Tensor | None = None

    def __call__(self, scores: torch.Tensor, k: int,
                 ext_hist1: torch.Tensor | None = None,
                 mask: torch.Tensor | None = None,
                 row_pred: torch.Tensor | None = None
                 ) -> tuple[torch.Tensor, torch.Tensor]:
        """mask [P, W] i32 (filter_bitmask) + row_pred [B] i32 select
        among passing documents only: row b honours mask[row_pred[b]];
        rows with fewer than k passing documents pad with -inf / -1."""
        assert scores.dim() == 2
        _check(scores, torch.float32, "scores")
        B, N = scores.shape
        assert 1 <= k <= 1024
        assert (mask is None) == (row_pred is None), \
            "mask and row_pred go together"
        if mask is not None:
            # a producer histogram counts failing documents too
            assert ext_hist1 is None, "ext_hist1 cannot be masked"
            _check(mask, torch.int32, "mask")
            _check(row_pred, torch.int32, "row_pred")
            assert mask.dim() == 2 and mask.shape[1] * 32 >= N
            assert row_pred.numel() == B
        if ext_hist1 is not None:
            # producer-fused pass 1 (bm25_block hist1=): exact counts
            assert ext_hist1.dtype == torch.int32 \
                and ext_hist1.numel() >= B * 256
        lib = _ext.lib()
        nu32 = lib.infomesh_topk_workspace_u32(B)
        if self._ws is None or self._ws.numel() < nu32:
            self._ws = torch.empty(nu32, device=scores.device,
                                   dtype=torch.int32)
        self._ws[:lib.infomesh_topk_zero_u32(B)].zero_()
        vals = torch.empty((B, k), device=scores.device, dtype=torch.float32)
        idx = torch.empty((B, k), device=scores.device, dtype=torch.int32)
        if mask is not None:
            lib.infomesh_topk_masked(
                scores.data_ptr(), self._ws.data_ptr(), vals.data_ptr(),
                idx.data_ptr(), B, N, k, mask.data_ptr(),
                row_pred.data_ptr(), mask.shape[1], _ext.stream_ptr())
            return vals, idx
        lib.infomesh_topk(scores.data_ptr(), self._ws.data_ptr(),
                          vals.data_ptr(), idx.data_ptr(), B, N, k,
                          0 if ext_hist1 is None else ext_hist1.data_ptr(),
                          _ext.stream_ptr())
        return vals, idx


class TopKPruned:
    """TopK for scores whose producer also wrote block maxima
    (gemm_nt_bmax, bm25_block(bmax=)): one kernel, one workgroup per
    row, that reads the [B, NB] maxima and k blocks of W scores per row
    instead of streaming [B, N] three times (infomesh_topk_pruned in
    csrc/topk.hip). No fill, and a workspace only for rows of more than
    24 576 block maxima (grouped maxima, kept across calls; one
    instance per captured graph). Its contract is stronger than TopK's:
    the first k of a stable descending sort of the row, so ties at rank
    k go to the lowest columns."""

    def __init__(self, device: torch.device | str = "cuda"):
        self.device = torch.device(device)
        self._ws: torch.Tensor | None = None

    def __call__(self, scores: torch.Tensor, bmax: torch.Tensor, W: int,
                 k: int) -> tuple[torch.Tensor, torch.Tensor]:
        assert scores.dim() == 2
        _check(scores, torch.float32, "scores")
        _check(bmax, torch.float32, "bmax")
        B, N = scores.shape
        assert 1 <= k <= 1024 and 0 < W <= 1 << 20
        assert bmax.shape == (B, (N + W - 1) // W), \
            f"bmax must be [B, ceil(N/W)], got {tuple(bmax.shape)}"
        vals = torch.empty((B, k), device=scores.device, dtype=torch.float32)
        idx = torch.empty((B, k), device=scores.device, dtype=torch.int32)
        lib = _ext.lib()
        nu32 = lib.infomesh_topk_pruned_workspace_u32(B, N, k, W)
        if nu32 and (self._ws is None or self._ws.numel() < nu32):
            self._ws = torch.empty(nu32, device=scores.device,
                                   dtype=torch.int32)
        rc = lib.infomesh_topk_pruned(
            scores.data_ptr(), bmax.data_ptr(), W,
            self._ws.data_ptr() if nu32 else 0,
            vals.data_ptr(), idx.data_ptr(), B, N, k, _ext.stream_ptr())
        assert rc == 0, f"topk_pruned: {N} columns at W = {W} is too wide"
        return vals, idx


def topk(scores: torch.Tensor, k: int) -> tuple[torch.Tensor, torch.Tensor]:
    return TopK(scores.device)(scores, k)


def filter_bitmask(attrs: torch.Tensor, preds: torch.Tensor) -> torch.Tensor:
    """Per-document attribute records [N, 4] i32 x predicates [P, 4] i32
    (index/doc_attrs.py, layout in csrc/docfilter.hip) -> pass bitmask
    [P, W] i32, W = ceil(N/64)*2; bit d&31 of word d>>5 is document d,
    bits at positions >= N are 0."""
    _check(attrs, torch.int32, "attrs")
    _check(preds, torch.int32, "preds")
    assert attrs.dim() == 2 and attrs.shape[1] == 4
    assert preds.dim() == 2 and preds.shape[1] == 4 and preds.shape[0] >= 1
    N, P = attrs.shape[0], preds.shape[0]
    assert P <= 65535
    W = (N + 63) // 64 * 2
    bits = torch.empty((P, W), device=attrs.device, dtype=torch.int32)
    _ext.lib().infomesh_filter_bitmask(
        attrs.data_ptr(), preds.data_ptr(), bits.data_ptr(), N, P,
        _ext.stream_ptr())
    return bits


FILTER_SETS_MAX = 2048   # hashes per predicate the kernel stages in LDS


def filter_bitmask_sets(attrs: torch.Tensor, preds: torch.Tensor,
                        desc: torch.Tensor, doms: torch.Tensor
                        ) -> torch.Tensor:
    """filter_bitmask with per-predicate domain lists: desc [P, 4] i32
    (allow_off, allow_n, block_off, block_n, offsets into doms) and doms
    the flat i32 array of u32 domain hashes, each list unique and
    ascending as unsigned (index/doc_attrs.pack_pred_sets). Same output.

    The descriptors are checked here, on the host, before the kernel
    indexes doms with them: hand desc over as a host tensor (it is then
    uploaded, no sync) or as a device tensor (copied back to check)."""
    _check(attrs, torch.int32, "attrs")
    _check(preds, torch.int32, "preds")
    assert attrs.dim() == 2 and attrs.shape[1] == 4
    assert preds.dim() == 2 and preds.shape[1] == 4 and preds.shape[0] >= 1
    N, P = attrs.shape[0], preds.shape[0]
    assert P <= 65535
    assert desc.dtype == torch.int32 and desc.shape == (P, 4) \
        and desc.is_contiguous(), "desc: contiguous [P, 4] i32"
    _check(doms, torch.int32, "doms")
    assert doms.dim() == 1
    h = desc.cpu()
    off, n = h[:, 0::2].long(), h[:, 1::2].long()
    assert bool((n >= 0).all()) and bool((off >= 0).all()) \
        and bool((off + n <= doms.numel()).all()), "desc points outside doms"
    assert int(n.sum(1).max()) <= FILTER_SETS_MAX, \
        f"more than {FILTER_SETS_MAX} hashes in one predicate's lists"
    if not desc.is_cuda:
        desc = desc.to(attrs.device, non_blocking=True)
    W = (N + 63) // 64 * 2
    bits = torch.empty((P, W), device=attrs.device, dtype=torch.int32)
    _ext.lib().infomesh_filter_bitmask_sets(
        attrs.data_ptr(), preds.data_ptr(), desc.data_ptr(),
        doms.data_ptr(), bits.data_ptr(), N, P, _ext.stream_ptr())
    return bits


TERM_OPS_MAX = 16   # operands per term row (csrc/termmask.hip)


def term_block_docs() -> int:
    """Documents per workgroup of term_bitmask (TERM_BLOCK)."""
    return int(_ext.lib().infomesh_term_block_docs())


def _host_i64(t: torch.Tensor, name: str, n: int) -> torch.Tensor:
    assert t.dtype == torch.int64 and t.shape == (n,) and t.is_contiguous(), \
        f"{name}: contiguous [{n}] i64"
    return t.cpu()


def term_bitmask(base_bits: torch.Tensor, src_row: torch.Tensor,
                 segments, op_off: torch.Tensor, op_kind: torch.Tensor,
                 N: int) -> torch.Tensor:
    """Required / excluded terms -> pass bits (csrc/termmask.hip, where
    the layout is written down). Term row r starts from
    base_bits[src_row[r]] ([P, W] i32, W = ceil(N/64)*2, as
    filter_bitmask writes them) and keeps document d's bit iff every
    require operand of the row has a posting for d and no exclude
    operand has one. Returns out [R, W] i32; base_bits is not written.

    op_off [R+1] i32: per-row CSR into the operand arrays, at most
    TERM_OPS_MAX operands per row; op_kind [T] i32, 0 = require,
    1 = exclude. segments: one (doc_ids, doc_base, nseg, op_begin,
    op_end) per posting segment, in any order: doc_ids the segment's
    i32 ids (segment-local, ascending per term), op_begin / op_end [T]
    i64 each operand's posting range in it (begin == end: term absent).
    The segments' document ranges must not overlap and lie inside
    [0, N).

    The table is checked here, on the host, before a kernel indexes with
    it: hand op_off, op_kind, op_begin and op_end over as host tensors
    (they are then uploaded, no sync) or as device tensors (copied back
    to check). One launch per segment, in stream order."""
    _check(base_bits, torch.int32, "base_bits")
    dev = base_bits.device
    W = (N + 63) // 64 * 2
    assert N >= 1 and base_bits.dim() == 2 and base_bits.shape[1] == W, \
        "base_bits: [P, ceil(N/64)*2]"
    P = base_bits.shape[0]
    assert src_row.dim() == 1 and src_row.dtype in (torch.int32, torch.int64)
    R = src_row.numel()
    assert 1 <= R <= 0x7FFFFFFF
    h_src = src_row.cpu().long()
    assert bool((h_src >= 0).all()) and bool((h_src < P).all()), \
        "src_row points outside base_bits"
    assert op_off.dtype == torch.int32 and op_off.shape == (R + 1,) \
        and op_off.is_contiguous(), "op_off: contiguous [R+1] i32"
    assert op_kind.dtype == torch.int32 and op_kind.dim() == 1 \
        and op_kind.is_contiguous(), "op_kind: contiguous [T] i32"
    T = op_kind.numel()
    h_off = op_off.cpu().long()
    n_ops = h_off.diff()
    assert int(h_off[0]) == 0 and bool((n_ops >= 0).all()) \
        and int(h_off[-1]) == T, "op_off: ascending CSR over the T operands"
    assert int(n_ops.max()) <= TERM_OPS_MAX, \
        f"more than {TERM_OPS_MAX} operands in one row"
    h_kind = op_kind.cpu()
    assert bool(((h_kind == 0) | (h_kind == 1)).all()), "op_kind: 0 or 1"
    spans = []
    for doc_ids, doc_base, nseg, op_begin, op_end in segments:
        _check(doc_ids, torch.int32, "doc_ids")
        assert doc_ids.dim() == 1
        hb = _host_i64(op_begin, "op_begin", T)
        he = _host_i64(op_end, "op_end", T)
        assert bool((hb >= 0).all()) and bool((hb <= he).all()) \
            and bool((he <= doc_ids.numel()).all()), \
            "operand range outside doc_ids"
        assert 0 <= doc_base and nseg >= 0 and doc_base + nseg <= N, \
            "segment outside [0, N)"
        if nseg:
            spans.append((int(doc_base), int(doc_base + nseg)))
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), \
        "segments overlap"
    out = base_bits.index_select(0, src_row.to(dev).long())
    if T == 0:
        return out
    off_d = op_off.to(dev, non_blocking=True)
    kind_d = op_kind.to(dev, non_blocking=True)
    lib = _ext.lib()
    for doc_ids, doc_base, nseg, op_begin, op_end in segments:
        if nseg == 0:
            continue
        b_d = op_begin.to(dev, non_blocking=True)
        e_d = op_end.to(dev, non_blocking=True)
        lib.infomesh_term_bitmask(
            doc_ids.data_ptr(), doc_ids.numel(), off_d.data_ptr(),
            b_d.data_ptr(), e_d.data_ptr(), kind_d.data_ptr(), T,
            out.data_ptr(), R, W, N, int(doc_base), int(nseg),
            _ext.stream_ptr())
    return out


FACET_MAX_EDGES = 7     # design limits of csrc/facets.hip
FACET_MAX_LANGS = 32
FACET_MAX_DOMS = 64
_FACET_GROUPS = ("total", "date_zero", "date0", "lang_zero", "lang0",
                 "lang_other", "dom0")


def facet_chunk_docs() -> int:
    """Documents per workgroup of facet_counts (FACET_CHUNK)."""
    return int(_ext.lib().infomesh_facet_chunk_docs())


def facet_slots(E: int, L: int) -> dict[str, int]:
    """First slot of every group of a facet_counts row, as the extension
    reports them (the layout is written down in csrc/facets.hip)."""
    lib = _ext.lib()
    return {name: int(lib.infomesh_facet_slot(i, E, L))
            for i, name in enumerate(_FACET_GROUPS)}


def facet_width(E: int, L: int, Dw: int) -> int:
    """Row width F of facet_counts' result."""
    return int(_ext.lib().infomesh_facet_width(E, L, Dw))


def _host_words(t: torch.Tensor, name: str) -> torch.Tensor:
    assert t.dtype == torch.int32 and t.is_contiguous(), \
        f"{name}: contiguous i32"
    return t.cpu()


def _match_rows(scores: torch.Tensor, rows: torch.Tensor,
                mask: torch.Tensor | None, row_pred: torch.Tensor | None,
                chunk_docs: int) -> tuple[int, int, int, int, int]:
    """The shared front of facet_counts, domain_count and domain_best:
    scores [B, N] f32 and, with a mask, mask [P, W] i32 + row_pred [B]
    i32, on the device; rows [R] i32 read on the host (a device tensor
    is copied back) and checked against B before a kernel indexes with
    it; at most 65535 chunks of chunk_docs documents, the grid's y
    limit. Returns (B, N, P, W, R); P = W = 0 without a mask."""
    _check(scores, torch.float32, "scores")
    assert scores.dim() == 2
    B, N = scores.shape
    assert N >= 1
    assert (mask is None) == (row_pred is None), \
        "mask and row_pred go together"
    W = P = 0
    if mask is not None:
        _check(mask, torch.int32, "mask")
        _check(row_pred, torch.int32, "row_pred")
        assert mask.dim() == 2 and mask.shape[1] * 32 >= N
        assert row_pred.numel() == B
        P, W = mask.shape
    h_rows = _host_words(rows, "rows")
    assert h_rows.dim() == 1 and h_rows.numel() >= 1, "rows: [R], R >= 1"
    assert bool(((h_rows >= 0) & (h_rows < B)).all()), \
        "rows points outside the batch"
    assert (N + chunk_docs - 1) // chunk_docs <= 65535
    return B, N, P, W, h_rows.numel()


def _zeroed(out: torch.Tensor | None, shape: tuple[int, ...],
            dtype: torch.dtype, device: torch.device) -> torch.Tensor:
    """The kernels' zeroed result: a fresh tensor, or the caller's
    contiguous device workspace `out` of that shape and dtype, zeroed."""
    if out is None:
        return torch.zeros(shape, device=device, dtype=dtype)
    _check(out, dtype, "out")
    assert out.shape == shape, f"out: {list(shape)}"
    out.zero_()
    return out


def facet_counts(scores: torch.Tensor, rows: torch.Tensor,
                 attrs: torch.Tensor, edges: torch.Tensor,
                 langs: torch.Tensor, dom_desc: torch.Tensor,
                 doms: torch.Tensor, mask: torch.Tensor | None = None,
                 row_pred: torch.Tensor | None = None) -> torch.Tensor:
    """Facet counts over every matching document (csrc/facets.hip, where
    the match rule and the slot layout are written down): scores [B, N]
    f32, attrs [N, 4] i32 and, with a mask, mask [P, W] i32 + row_pred
    [B] i32 as TopK takes them, on the device. rows [R] i32 names the
    batch rows to count; edges [E] and langs [L] hold u32 words as i32,
    ascending as unsigned (langs unique); dom_desc [R, 2] i32 is (off, n)
    of each counted row's list in doms, the flat i32 array of u32 domain
    hashes, each list unique and ascending as unsigned. Returns counts
    [R, F] i32, F = facet_width(E, L, max n); slots per facet_slots.

    rows, edges, langs, dom_desc and doms are checked here, on the host,
    before the kernel indexes with them: hand them over as host tensors
    (they are then uploaded, no sync) or as device tensors (copied back
    to check). More than 7 edges, 32 languages or 64 hashes in one list
    is a ValueError, and nothing is launched."""
    _check(attrs, torch.int32, "attrs")
    B, N, P, W, R = _match_rows(scores, rows, mask, row_pred,
                                facet_chunk_docs())
    assert attrs.shape == (N, 4), "attrs: [N, 4]"
    h_edges = _host_words(edges, "edges")
    h_langs = _host_words(langs, "langs")
    h_desc = _host_words(dom_desc, "dom_desc")
    h_doms = _host_words(doms, "doms")
    assert h_edges.dim() == 1 and h_langs.dim() == 1 and h_doms.dim() == 1
    E, L = h_edges.numel(), h_langs.numel()
    assert h_desc.shape == (R, 2), "dom_desc: [R, 2]"
    off, n = h_desc[:, 0].long(), h_desc[:, 1].long()
    assert bool((n >= 0).all()) and bool((off >= 0).all()) \
        and bool((off + n <= h_doms.numel()).all()), \
        "dom_desc points outside doms"
    Dw = int(n.max())
    if E > FACET_MAX_EDGES or L > FACET_MAX_LANGS or Dw > FACET_MAX_DOMS:
        raise ValueError(
            f"facets: {E} date edges, {L} languages, {Dw} domains in one "
            f"list; the caps are {FACET_MAX_EDGES}, {FACET_MAX_LANGS} and "
            f"{FACET_MAX_DOMS}")

    def asc(t, strict):
        u = t.long() & 0xFFFFFFFF
        d = u.diff()
        return bool((d > 0).all()) if strict else bool((d >= 0).all())
    assert asc(h_edges, False), "edges: ascending as unsigned"
    assert asc(h_langs, True), "langs: ascending and unique"
    assert all(asc(h_doms[o:o + c], True)
               for o, c in zip(off.tolist(), n.tolist())), \
        "doms: every list ascending as unsigned and unique"
    dev = scores.device
    tables = (dom_desc, rows, edges, langs, doms)
    if not any(t.is_cuda for t in tables):
        # one upload for the five host tables; dom_desc first, so that
        # its (off, n) pairs stay 8-byte aligned
        flat = torch.cat([t.reshape(-1) for t in tables]).to(
            dev, non_blocking=True)
        desc_d, rows_d, edges_d, langs_d, doms_d = flat.split(
            [t.numel() for t in tables])
    else:
        desc_d, rows_d, edges_d, langs_d, doms_d = (
            t if t.is_cuda else t.to(dev, non_blocking=True) for t in tables)
    F = facet_width(E, L, Dw)
    counts = torch.zeros((R, F), device=dev, dtype=torch.int32)
    _ext.lib().infomesh_facet_counts(
        scores.data_ptr(), rows_d.data_ptr(), _ptr(mask), _ptr(row_pred),
        attrs.data_ptr(), edges_d.data_ptr() if E else None,
        langs_d.data_ptr() if L else None, desc_d.data_ptr(),
        doms_d.data_ptr() if doms_d.numel() else None, doms_d.numel(),
        counts.data_ptr(), B, R, N, W, P, E, L, F, _ext.stream_ptr())
    return counts


def domtop_chunk_docs() -> int:
    """Documents per workgroup of domain_count (DOMTOP_CHUNK)."""
    return int(_ext.lib().infomesh_domtop_chunk_docs())


def domtop_lds_slots() -> int:
    """Slots of domain_count's per-workgroup LDS table."""
    return int(_ext.lib().infomesh_domtop_lds_slots())


def domtop_k_max() -> int:
    """The largest K domain_select takes."""
    return int(_ext.lib().infomesh_domtop_k_max())


def domain_count(scores: torch.Tensor, rows: torch.Tensor,
                 dom_id: torch.Tensor, D: int,
                 mask: torch.Tensor | None = None,
                 row_pred: torch.Tensor | None = None,
                 out: torch.Tensor | None = None) -> torch.Tensor:
    """Matching documents per domain id (csrc/domtop.hip; the match rule
    is the one of facet_counts): scores [B, N] f32, dom_id [N] i32 with
    every entry in [0, D) and, with a mask, mask [P, W] i32 + row_pred
    [B] i32, on the device. rows [R] i32 names the batch rows to count
    and is checked here, on the host, before the kernel indexes with it
    (a host tensor is uploaded, a device tensor copied back). out: a
    contiguous [R, D] i32 device tensor to count into; it is zeroed
    here. Returns cnt [R, D] i32. dom_id is the caller's to keep inside
    [0, D): the kernel drops an id outside it."""
    _check(dom_id, torch.int32, "dom_id")
    if D < 1:
        raise ValueError(f"domain_count: D = {D}; at least one domain")
    B, N, P, W, R = _match_rows(scores, rows, mask, row_pred,
                                domtop_chunk_docs())
    assert dom_id.shape == (N,), "dom_id: [N]"
    dev = scores.device
    rows_d = rows if rows.is_cuda else rows.to(dev, non_blocking=True)
    out = _zeroed(out, (R, D), torch.int32, dev)
    _ext.lib().infomesh_domain_count(
        scores.data_ptr(), rows_d.data_ptr(), _ptr(mask), _ptr(row_pred),
        dom_id.data_ptr(), out.data_ptr(), B, R, N, W, P, D,
        _ext.stream_ptr())
    return out


def domain_select(cnt: torch.Tensor, dom_keys: torch.Tensor,
                  K: int) -> torch.Tensor:
    """The first K domains of every row of cnt [R, D] i32 (counts >= 0)
    by count descending, then id ascending (csrc/domtop.hip), as
    (dom_keys[id], count) pairs: [R, K, 2] i32. count > 0 marks a real
    entry; past the last one the pairs are (0, 0). dom_keys [D] i32. K
    outside 1 .. domtop_k_max() is a ValueError, and nothing is
    launched."""
    _check(cnt, torch.int32, "cnt")
    _check(dom_keys, torch.int32, "dom_keys")
    assert cnt.dim() == 2
    R, D = cnt.shape
    if not 1 <= K <= domtop_k_max():
        raise ValueError(
            f"domain_select: K = {K}; 1 <= K <= {domtop_k_max()}")
    if D < 1:
        raise ValueError(f"domain_select: D = {D}; at least one domain")
    assert R >= 1 and dom_keys.shape == (D,), "dom_keys: [D]"
    out = torch.empty((R, K, 2), device=cnt.device, dtype=torch.int32)
    _ext.lib().infomesh_domain_select(
        cnt.data_ptr(), dom_keys.data_ptr(), out.data_ptr(), R, D, K,
        _ext.stream_ptr())
    return out


def collapse_m_max() -> int:
    """The largest per-domain cap m (COLLAPSE_M_MAX)."""
    return int(_ext.lib().infomesh_collapse_m_max())


def collapse_k_max() -> int:
    """The largest k collapse_select takes."""
    return int(_ext.lib().infomesh_collapse_k_max())


def collapse_chunk_docs() -> int:
    """Documents per workgroup of domain_best (COLLAPSE_CHUNK)."""
    return int(_ext.lib().infomesh_collapse_chunk_docs())


def collapse_lds_slots() -> int:
    """Slots of domain_best's per-workgroup LDS table."""
    return int(_ext.lib().infomesh_collapse_lds_slots())


def domain_best(scores: torch.Tensor, rows: torch.Tensor,
                dom_id: torch.Tensor, D: int, m: int, positive: bool,
                mask: torch.Tensor | None = None,
                row_pred: torch.Tensor | None = None,
                out: torch.Tensor | None = None,
                rows_device: torch.Tensor | None = None) -> torch.Tensor:
    """The m best eligible documents of every domain id, as order keys
    (csrc/collapse.hip, where the key and the order are written down):
    scores [B, N] f32, dom_id [N] i32 with every entry in [0, D) and,
    with a mask, mask [P, W] i32 + row_pred [B] i32, on the device.
    positive: the BM25 form, eligible = passes the mask and score > 0
    (facet_counts' rule); else the dense form, eligible = passes the
    mask. rows [R] i32 names the batch rows and is checked here, on the
    host, before any launch (a host tensor is uploaded, a device tensor
    copied back). rows_device: the device copy of a host `rows`, from a
    caller that has uploaded it already. out: a contiguous [m, R, D] i64
    device tensor to fill; it is zeroed here. Returns best [m, R, D] i64 holding the u64 keys'
    bits: best[j, r, i] is the (j+1)-th largest key of domain i in row
    rows[r], 0 when the domain has no such document. m outside
    1 .. collapse_m_max() is a ValueError, and nothing is launched."""
    _check(dom_id, torch.int32, "dom_id")
    if not 1 <= m <= collapse_m_max():
        raise ValueError(
            f"domain_best: m = {m}; 1 <= m <= {collapse_m_max()}")
    if D < 1:
        raise ValueError(f"domain_best: D = {D}; at least one domain")
    N = scores.shape[-1]
    if (N + collapse_chunk_docs() - 1) // collapse_chunk_docs() > 65535:
        raise ValueError(f"domain_best: N = {N}; more than 65535 chunks")
    B, N, P, W, R = _match_rows(scores, rows, mask, row_pred,
                                collapse_chunk_docs())
    assert N < 2 ** 31 and dom_id.shape == (N,), "dom_id: [N]"
    dev = scores.device
    if rows_device is not None:
        assert not rows.is_cuda and rows_device.is_cuda \
            and rows_device.dtype == torch.int32 \
            and rows_device.shape == rows.shape, "rows_device: rows, uploaded"
        rows_d = rows_device
    else:
        rows_d = rows if rows.is_cuda else rows.to(dev, non_blocking=True)
    out = _zeroed(out, (m, R, D), torch.int64, dev)
    _ext.lib().infomesh_domain_best(
        scores.data_ptr(), rows_d.data_ptr(), _ptr(mask), _ptr(row_pred),
        dom_id.data_ptr(), out.data_ptr(), B, R, N, W, P, D, m,
        1 if positive else 0, _ext.stream_ptr())
    return out


def collapse_select(best: torch.Tensor, k: int
                    ) -> tuple[torch.Tensor, torch.Tensor]:
    """The first k documents of every row's capped set, in key order
    (csrc/collapse.hip): best [m, R, D] i64 as domain_best returns it ->
    (vals [R, k] f32, idx [R, k] i32), padded with -inf / -1. k outside
    1 .. collapse_k_max() is a ValueError, and nothing is launched."""
    _check(best, torch.int64, "best")
    assert best.dim() == 3
    m, R, D = best.shape
    if not 1 <= m <= collapse_m_max():
        raise ValueError(
            f"collapse_select: m = {m}; 1 <= m <= {collapse_m_max()}")
    if not 1 <= k <= collapse_k_max():
        raise ValueError(
            f"collapse_select: k = {k}; 1 <= k <= {collapse_k_max()}")
    assert R >= 1 and D >= 1, "best: [m, R, D]"
    vals = torch.empty((R, k), device=best.device, dtype=torch.float32)
    idx = torch.empty((R, k), device=best.device, dtype=torch.int32)
    _ext.lib().infomesh_collapse_select(
        best.data_ptr(), vals.data_ptr(), idx.data_ptr(), R, D, m, k,
        _ext.stream_ptr())
    return vals, idx


def bm25_block(doc_ids: torch.Tensor, tfdl: torch.Tensor,
               qt_off: torch.Tensor, qt_ut: torch.Tensor,
               qt_idf: torch.Tensor, u_begin: torch.Tensor,
               u_end: torch.Tensor, bounds: torch.Tensor,
               scores: torch.Tensor, doc_base: int, nseg: int,
               bd: int, avgdl: float, k1: float = 1.2,
               b: float = 0.75,
               hist1: torch.Tensor | None = None,
               bmax: torch.Tensor | None = None) -> torch.Tensor:
    """Doc-block LDS-accumulated BM25 for ONE posting segment.

    Two launches: a bounds pre-pass binary-searching each (unique term,
    doc-block) posting sub-range once, then the block kernel (one
    workgroup per (query, doc-block), query-major so adjacent
    workgroups reuse posting reads through L2). Writes every element of
    scores[:, doc_base:doc_base+nseg] exactly once (zero where no
    posting hits) — no pre-zeroing needed when segments partition the
    doc axis. Norm is computed in-kernel from the packed per-posting
    doc length and the current global avgdl.

    bounds: caller-provided i32 workspace of at least
    U * ceil(nseg/bd) * 2 elements.

    bmax (instead of hist1): [B, ceil(N/64)] f32; the kernel also writes
    the maximum of every block of 64 columns it writes, for
    TopKPruned(scores, bmax, 64, k). Needs doc_base % 64 == 0, so that
    no block straddles two segments."""
    B, N = scores.shape
    U = u_begin.numel()
    nblocks = (nseg + bd - 1) // bd
    _check(scores, torch.float32, "scores")
    assert nblocks <= 65535 and qt_off.numel() == B + 1
    assert doc_ids.dtype == torch.int32 and tfdl.dtype == torch.int32
    assert bounds.numel() >= U * nblocks * 2
    # 8448 B = HIST8_U32 (common.h) u32 histogram copies after the tile
    assert bd * 4 + (8448 if hist1 is not None else 0) <= 160 * 1024
    if hist1 is not None:
        # fused topk pass 1: exact [B,256] ordered-top-byte counts of the
        # written score columns (caller zeroes it before the first
        # segment and hands it to topk(ext_hist1=...))
        assert hist1.dtype == torch.int32 and hist1.numel() >= B * 256
    if bmax is not None:
        assert hist1 is None, "bmax and hist1 are mutually exclusive"
        _check(bmax, torch.float32, "bmax")
        assert bmax.shape == (B, (N + 63) // 64), \
            f"bmax must be [B, ceil(N/64)], got {tuple(bmax.shape)}"
        assert doc_base % 64 == 0 and bd % 64 == 0, \
            "bmax: segment base and doc-block must be multiples of 64"
    norm_a = k1 * (1.0 - b)
    norm_b = k1 * b / max(avgdl, 1e-9)
    lib = _ext.lib()
    if bmax is not None:
        fn, side = lib.infomesh_bm25_block_bmax, bmax.data_ptr()
    else:
        fn = lib.infomesh_bm25_block
        side = 0 if hist1 is None else hist1.data_ptr()
    fn(
        doc_ids.data_ptr(), tfdl.data_ptr(), qt_off.data_ptr(),
        qt_ut.data_ptr(), qt_idf.data_ptr(), u_begin.data_ptr(),
        u_end.data_ptr(), bounds.data_ptr(), scores.data_ptr(), side,
        B, U, N, doc_base, nseg, bd,
        norm_a, norm_b, k1 + 1.0, _ext.stream_ptr())
    return scores


def score_combine(a: torch.Tensor, b: torch.Tensor, wa: float,
                  wb: float) -> torch.Tensor:
    out = torch.empty_like(a)
    _ext.lib().infomesh_score_combine(a.data_ptr(), b.data_ptr(),
                                      out.data_ptr(), wa, wb, a.numel(),
                                      _ext.stream_ptr())
    return out


def simhash_fingerprint(offsets: torch.Tensor,
                        hashes: torch.Tensor) -> torch.Tensor:
    """CSR shingle hashes (int64-as-u64) -> int64 fingerprints [D]."""
    ndocs = offsets.numel() - 1
    out = torch.empty(ndocs, device=offsets.device, dtype=torch.int64)
    _ext.lib().infomesh_simhash_fingerprint(
        offsets.data_ptr(), hashes.data_ptr(), out.data_ptr(), ndocs,
        _ext.stream_ptr())
    return out


def hamming_scan(queries: torch.Tensor, table: torch.Tensor,
                 radius: int = 3, cap: int = 65536
                 ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Matches (q_idx, table_idx, dist) with hamming(q, t) <= radius."""
    M, N = queries.numel(), table.numel()
    dev = table.device
    out_q = torch.empty(cap, device=dev, dtype=torch.int32)
    out_n = torch.empty(cap, device=dev, dtype=torch.int32)
    out_d = torch.empty(cap, device=dev, dtype=torch.int32)
    cnt = torch.zeros(1, device=dev, dtype=torch.int32)
    _ext.lib().infomesh_hamming_scan(
        queries.data_ptr(), table.data_ptr(), out_q.data_ptr(),
        out_n.data_ptr(), out_d.data_ptr(), cnt.data_ptr(), M, N, radius,
        cap, _ext.stream_ptr())
    n = min(int(cnt.item()), cap)
    return out_q[:n], out_n[:n], out_d[:n]


def attn_fused(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
               valid_len: torch.Tensor | None = None,
               causal: bool = False, scale: float | None = None,
               out: torch.Tensor | None = None, variant: int = 0
               ) -> torch.Tensor | None:
    """Fused flash attention: q [B,nh,Sq,d], k/v [B,nhk,Sk,d] — any
    batch/head/row strides (element stride must be 1, d in {32,64,96,
    128}). GQA via nh % nhk == 0. valid_len: [B] i32 key limits.
    Returns O [B*nh, Sq, d] bf16 contiguous, or, given out= (a
    [B,nh,Sq,d] bf16 view with element stride 1 and any other strides,
    e.g. the head view of a merged [B*Sq, nh*d] buffer), writes there
    and returns it. variant: 0 = the kernel's own choice, 1 = the
    general 64x64 tile, 2 = the short 32x32 tile, which gives the same
    bits and covers only Sq <= 32 and Sk <= 32: None, with nothing
    launched, when asked for anything else."""
    assert q.dim() == 4 and k.dim() == 4 and v.dim() == 4
    B, nh, Sq, d = q.shape
    _, nhk, Sk, dk = k.shape
    assert d == dk and d in (32, 64, 96, 128) and nh % nhk == 0
    for t in (q, k, v):
        assert t.dtype == torch.bfloat16 and t.stride(3) == 1
    if scale is None:
        scale = d ** -0.5
    assert k.shape[0] == B and v.shape == k.shape and Sq >= 1 and Sk >= 1
    if out is None:
        ret = torch.empty(B * nh, Sq, d, device=q.device,
                          dtype=torch.bfloat16)
        ostr = (nh * Sq * d, Sq * d, d)
        optr = ret.data_ptr()
    else:
        assert out.shape == (B, nh, Sq, d) and out.is_cuda
        assert out.dtype == torch.bfloat16 and out.stride(3) == 1
        ret, ostr, optr = out, out.stride()[:3], out.data_ptr()
    if valid_len is not None:
        _check(valid_len, torch.int32, "valid_len")
        assert valid_len.numel() == B
    rc = _ext.lib().infomesh_attn_fused(
        q.data_ptr(), k.data_ptr(), v.data_ptr(), _ptr(valid_len),
        optr, B, nh, nhk, Sq, Sk, d,
        q.stride(0), q.stride(1), q.stride(2),
        k.stride(0), k.stride(1), k.stride(2),
        v.stride(0), v.stride(1), v.stride(2),
        ostr[0], ostr[1], ostr[2],
        int(causal), scale, variant, _ext.stream_ptr())
    return ret if rc == 0 else None


def attn_decode(q: torch.Tensor, k_cache: torch.Tensor,
                v_cache: torch.Tensor, lens: torch.Tensor,
                scale: float) -> torch.Tensor:
    """q [B,H,D], caches [B,Hkv,Smax,D], lens [B] i32 -> out [B,H,D].

    Uses flash-decoding sequence splitting when B*H alone cannot fill
    the chip (partials per chunk + combine kernel)."""
    import math
    B, H, D = q.shape
    _, Hkv, Smax, _ = k_cache.shape
    _check(q, torch.bfloat16, "q")
    assert D % 8 == 0 and D <= 128
    out = torch.empty_like(q)
    nc_min = max(1, math.ceil(Smax / 2048))
    nc = max(nc_min, min(64, math.ceil(512 / max(1, B * H))))
    if nc <= 1:
        _ext.lib().infomesh_attn_decode(
            q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
            lens.data_ptr(), out.data_ptr(), B, H, Hkv, Smax, D, scale,
            _ext.stream_ptr())
    else:
        part = torch.empty(B, H, nc, D + 2, device=q.device,
                           dtype=torch.float32)
        _ext.lib().infomesh_attn_decode_split(
            q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
            lens.data_ptr(), part.data_ptr(), out.data_ptr(),
            B, H, Hkv, Smax, D, nc, scale, _ext.stream_ptr())
    return out


def qkv_split(qkv: torch.Tensor, B: int, S: int, nh: int, nkv: int,
              d: int, cos_t: torch.Tensor | None = None,
              sin_t: torch.Tensor | None = None,
              pos: torch.Tensor | None = None,
              rot: int | None = None, want_vt: bool = True
              ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor | None]:
    """Fused head split (+RoPE on q/k when tables given):
    qkv [B*S, (nh+2nkv)*d] -> q [B*nh,S,d], k [B*nkv,S,d], and (when
    want_vt) the PV-GEMM-ready transposed vt [B*nkv,d,S]; the fused
    attention path reads V strided from qkv instead (want_vt=False)."""
    _check(qkv, torch.bfloat16, "qkv")
    dev = qkv.device
    q = torch.empty(B * nh, S, d, device=dev, dtype=torch.bfloat16)
    k = torch.empty(B * nkv, S, d, device=dev, dtype=torch.bfloat16)
    vt = torch.empty(B * nkv, d, S, device=dev, dtype=torch.bfloat16) \
        if want_vt else None
    _ext.lib().infomesh_qkv_split(
        qkv.data_ptr(), q.data_ptr(), k.data_ptr(), _ptr(vt),
        _ptr(cos_t), _ptr(sin_t), _ptr(pos),
        B, S, nh, nkv, d, rot or d, _ext.stream_ptr())
    return q, k, vt


def merge_heads(ctx: torch.Tensor, B: int, S: int, nh: int,
                d: int) -> torch.Tensor:
    """[B*nh, S, d] -> [B*S, nh*d]."""
    _check(ctx, torch.bfloat16, "ctx")
    out = torch.empty(B * S, nh * d, device=ctx.device, dtype=torch.bfloat16)
    _ext.lib().infomesh_merge_heads(ctx.data_ptr(), out.data_ptr(),
                                    B, S, nh, d, _ext.stream_ptr())
    return out


def silu_mul_fused(gu: torch.Tensor, F: int) -> torch.Tensor:
    """gu [rows, 2F] -> silu(gu[:, :F]) * gu[:, F:] without slicing."""
    _check(gu, torch.bfloat16, "gu")
    rows = gu.shape[0]
    assert gu.shape[1] == 2 * F and F % 8 == 0
    out = torch.empty(rows, F, device=gu.device, dtype=torch.bfloat16)
    _ext.lib().infomesh_silu_mul_fused(gu.data_ptr(), out.data_ptr(),
                                       rows, F, _ext.stream_ptr())
    return out


def kv_append(k_new: torch.Tensor, v_new: torch.Tensor,
              k_cache: torch.Tensor, v_cache: torch.Tensor,
              pos: torch.Tensor) -> None:
    B, Hkv, D = k_new.shape
    _, _, Smax, _ = k_cache.shape
    _ext.lib().infomesh_kv_append(
        k_new.data_ptr(), v_new.data_ptr(), k_cache.data_ptr(),
        v_cache.data_ptr(), pos.data_ptr(), B, Hkv, Smax, D,
        _ext.stream_ptr())
