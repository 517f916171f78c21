"""ctypes loader for the CDNA4 HIP extension (fail-loud policy).

On a machine with a GPU the extension MUST load — ops raise
GpuExtensionMissing rather than silently falling back to eager PyTorch
(the round-end check records which .so files the GPU processes load).
On CPU-only machines the torch reference implementations in
ops/reference.py are the test oracle instead.
"""
from __future__ import annotations

import ctypes
from ctypes import c_float, c_int, c_long, c_void_p
from pathlib import Path

from ..errors import GpuExtensionMissing

_LIB: ctypes.CDLL | None = None
_LOAD_ERROR: str | None = None

_SIGNATURES: dict[str, list] = {
    "infomesh_gemm_bf16_nt": [c_void_p, c_void_p, c_void_p, c_void_p,
                              c_int, c_int, c_int, c_int,
                              c_long, c_long, c_long,
                              c_int, c_float, c_int, c_void_p],
    "infomesh_layernorm": [c_void_p, c_void_p, c_void_p, c_void_p,
                           c_void_p, c_void_p, c_long, c_int, c_float,
                           c_long, c_void_p],
    "infomesh_embed_layernorm": [c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_long, c_int, c_int,
                                 c_float, c_void_p],
    "infomesh_rmsnorm": [c_void_p, c_void_p, c_void_p, c_void_p,
                         c_void_p, c_long, c_int, c_float, c_void_p],
    "infomesh_softmax": [c_void_p, c_void_p, c_void_p, c_long, c_int,
                         c_int, c_int, c_float, c_void_p],
    "infomesh_bias_act": [c_void_p, c_void_p, c_long, c_int, c_int, c_void_p],
    "infomesh_silu_mul": [c_void_p, c_void_p, c_void_p, c_long, c_void_p],
    "infomesh_add": [c_void_p, c_void_p, c_void_p, c_long, c_void_p],
    "infomesh_rope": [c_void_p, c_void_p, c_void_p, c_void_p, c_long,
                      c_int, c_int, c_int, c_void_p],
    "infomesh_gather": [c_void_p, c_void_p, c_void_p, c_long, c_int,
                        c_float, c_void_p],
    "infomesh_pool": [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                      c_int, c_int, c_void_p],
    "infomesh_argmax": [c_void_p, c_void_p, c_long, c_int, c_void_p],
    "infomesh_topk": [c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                      c_long, c_int, c_void_p, c_void_p],
    "infomesh_topk_masked": [c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                             c_long, c_int, c_void_p, c_void_p, c_long,
                             c_void_p],
    "infomesh_filter_bitmask": [c_void_p, c_void_p, c_void_p, c_long,
                                c_int, c_void_p],
    "infomesh_filter_bitmask_sets": [c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_long, c_int, c_void_p],
    "infomesh_term_bitmask": [c_void_p, c_long, c_void_p, c_void_p,
                              c_void_p, c_void_p, c_int, c_void_p, c_int,
                              c_long, c_long, c_long, c_long, c_void_p],
    "infomesh_term_block_docs": [],
    "infomesh_topk_workspace_u32": [c_int],
    "infomesh_topk_zero_u32": [c_int],
    "infomesh_bm25_block": [c_void_p, c_void_p, c_void_p, c_void_p,
                            c_void_p, c_void_p, c_void_p, c_void_p,
                            c_void_p, c_void_p, c_int, c_int, c_long,
                            c_long, c_long, c_int, c_float, c_float,
                            c_float, c_void_p],
    "infomesh_bm25_block_bmax": [c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_int, c_int, c_long,
                                 c_long, c_long, c_int, c_float, c_float,
                                 c_float, c_void_p],
    "infomesh_score_combine": [c_void_p, c_void_p, c_void_p, c_float,
                               c_float, c_long, c_void_p],
    "infomesh_simhash_fingerprint": [c_void_p, c_void_p, c_void_p, c_long,
                                     c_void_p],
    "infomesh_hamming_scan": [c_void_p, c_void_p, c_void_p, c_void_p,
                              c_void_p, c_void_p, c_int, c_long, c_int,
                              c_int, c_void_p],
    "infomesh_attn_decode": [c_void_p, c_void_p, c_void_p, c_void_p,
                             c_void_p, c_int, c_int, c_int, c_int, c_int,
                             c_float, c_void_p],
    "infomesh_attn_decode_split": [c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_int, c_int, c_int,
                                   c_int, c_int, c_int, c_float, c_void_p],
    "infomesh_attn_fused": [c_void_p, c_void_p, c_void_p, c_void_p,
                            c_void_p, c_int, c_int, c_int, c_int, c_int,
                            c_int, c_long, c_long, c_long, c_long, c_long,
                            c_long, c_long, c_long, c_long,
                            c_long, c_long, c_long,
                            c_int, c_float, c_int, c_void_p],
    "infomesh_kv_append": [c_void_p, c_void_p, c_void_p, c_void_p,
                           c_void_p, c_int, c_int, c_int, c_int, c_void_p],
    "infomesh_dense_scores": [c_void_p, c_void_p, c_void_p,
                              c_int, c_long, c_int, c_float, c_void_p],
    "infomesh_dense_scores_fp8": [c_void_p, c_void_p, c_void_p,
                                  c_int, c_long, c_int, c_float,
                                  c_void_p],
    "infomesh_gemm8_bf16_nt": [c_void_p, c_void_p, c_void_p, c_void_p,
                               c_int, c_int, c_int, c_int,
                               c_long, c_long, c_long,
                               c_int, c_float, c_int, c_void_p],
    "infomesh_gemv_bf16_nt": [c_void_p, c_void_p, c_void_p, c_void_p,
                              c_int, c_int, c_int, c_int,
                              c_long, c_long, c_long,
                              c_int, c_float, c_int, c_void_p],
    "infomesh_qkv_split": [c_void_p, c_void_p, c_void_p, c_void_p,
                           c_void_p, c_void_p, c_void_p,
                           c_int, c_int, c_int, c_int, c_int, c_int,
                           c_void_p],
    "infomesh_merge_heads": [c_void_p, c_void_p, c_int, c_int, c_int,
                             c_int, c_void_p],
    "infomesh_silu_mul_fused": [c_void_p, c_void_p, c_long, c_int,
                                c_void_p],
    "infomesh_gemm_tile": [c_int, c_int, c_int, c_int],
    "infomesh_gemm_bmax_width": [c_int, c_int, c_int, c_int],
    "infomesh_gemm_bf16_nt_bmax": [c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_int, c_int, c_int, c_int,
                                   c_long, c_long, c_long,
                                   c_int, c_float, c_void_p],
    "infomesh_topk_pruned": [c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                             c_void_p, c_int, c_long, c_int, c_void_p],
    "infomesh_topk_pruned_workspace_u32": [c_int, c_long, c_int, c_int],
    "infomesh_facet_counts": [c_void_p, c_void_p, c_void_p, c_void_p,
                              c_void_p, c_void_p, c_void_p, c_void_p,
                              c_void_p, c_long, c_void_p, c_int, c_int,
                              c_long, c_long, c_int, c_int, c_int, c_int,
                              c_void_p],
    "infomesh_facet_chunk_docs": [],
    "infomesh_facet_width": [c_int, c_int, c_int],
    "infomesh_facet_slot": [c_int, c_int, c_int],
    "infomesh_domain_count": [c_void_p, c_void_p, c_void_p, c_void_p,
                              c_void_p, c_void_p, c_int, c_int, c_long,
                              c_long, c_int, c_int, c_void_p],
    "infomesh_domain_select": [c_void_p, c_void_p, c_void_p, c_int, c_int,
                               c_int, c_void_p],
    "infomesh_domtop_chunk_docs": [],
    "infomesh_domtop_lds_slots": [],
    "infomesh_domtop_k_max": [],
    "infomesh_domain_best": [c_void_p, c_void_p, c_void_p, c_void_p,
                             c_void_p, c_void_p, c_int, c_int, c_long,
                             c_long, c_int, c_int, c_int, c_int, c_void_p],
    "infomesh_collapse_select": [c_void_p, c_void_p, c_void_p, c_int, c_int,
                                 c_int, c_int, c_void_p],
    "infomesh_collapse_m_max": [],
    "infomesh_collapse_k_max": [],
    "infomesh_collapse_chunk_docs": [],
    "infomesh_collapse_lds_slots": [],
}

# Everything not listed here returns void. topk_*_u32: lengths;
# dense_scores, gemm_bf16_nt_bmax: dispatch eligibility (0 = launched);
# gemm_tile: tile code; gemm_bmax_width: columns per block maximum;
# attn_fused, embed_layernorm: 0 = launched, 1 = shape refused;
# term_block_docs: documents per workgroup of term_bitmask; facet_*: the
# chunk size and the slot layout of facet_counts; domtop_*: the chunk
# size, the LDS table size and the K cap of csrc/domtop.hip; collapse_*:
# the caps on m and k, the chunk size and the LDS table size of
# csrc/collapse.hip.
_RESTYPES = {"infomesh_topk_workspace_u32": c_long,
             "infomesh_collapse_m_max": c_int,
             "infomesh_collapse_k_max": c_int,
             "infomesh_collapse_chunk_docs": c_int,
             "infomesh_collapse_lds_slots": c_int,
             "infomesh_domtop_chunk_docs": c_int,
             "infomesh_domtop_lds_slots": c_int,
             "infomesh_domtop_k_max": c_int,
             "infomesh_facet_chunk_docs": c_int,
             "infomesh_facet_width": c_int,
             "infomesh_facet_slot": c_int,
             "infomesh_topk_zero_u32": c_long,
             "infomesh_topk_pruned": c_int,
             "infomesh_topk_pruned_workspace_u32": c_long,
             "infomesh_term_block_docs": c_int,
             "infomesh_gemm_bmax_width": c_int,
             "infomesh_gemm_bf16_nt_bmax": c_int,
             "infomesh_dense_scores": c_int,
             "infomesh_dense_scores_fp8": c_int,
             "infomesh_gemm_tile": c_int,
             "infomesh_attn_fused": c_int,
             "infomesh_embed_layernorm": c_int}


def bind(so: Path | str, strict: bool = True) -> ctypes.CDLL:
    """Load a build of the extension and type its entry points.
    strict=False skips the ones that build lacks: the probes under
    scripts/ time an older build beside the current one."""
    lib = ctypes.CDLL(str(so))
    for name, argtypes in _SIGNATURES.items():
        if not strict and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = _RESTYPES.get(name)
    return lib


def _try_load() -> ctypes.CDLL | None:
    global _LOAD_ERROR
    so = Path(__file__).resolve().parent / "libinfomesh_hip.so"
    if not so.exists():
        _LOAD_ERROR = f"{so} not built"
        return None
    try:
        lib = bind(so)
    except OSError as e:
        _LOAD_ERROR = str(e)
        return None
    import os
    if os.environ.get("INFOMESH_SYNC_DEBUG"):
        return _SyncDebugLib(lib)
    return lib


class _SyncDebugLib:
    """Sanitizer-style launch checking (INFOMESH_SYNC_DEBUG=1): after
    every kernel launch, synchronize the device so an async fault
    (bad pointer, OOB write surfacing later) raises AT THE LAUNCH SITE
    with the kernel's name, instead of poisoning a later op. The GPU
    analogue of the reference's structural concurrency checks
     — debugging only, serializes every launch."""

    def __init__(self, real: ctypes.CDLL):
        self._real = real

    def __getattr__(self, name: str):
        fn = getattr(self._real, name)
        if not name.startswith("infomesh_"):
            return fn

        def checked(*args, _fn=fn, _name=name):
            r = _fn(*args)
            import torch
            if torch.cuda.is_available():
                try:
                    torch.cuda.synchronize()
                except RuntimeError as e:
                    raise RuntimeError(
                        f"async GPU fault surfaced at {_name}: {e}"
                    ) from e
            return r
        return checked


def lib():
    """The loaded extension; raises GPU001 when missing."""
    global _LIB
    if _LIB is None:
        _LIB = _try_load()
    if _LIB is None:
        raise GpuExtensionMissing(_LOAD_ERROR or "unknown load failure")
    return _LIB


def available() -> bool:
    global _LIB
    if _LIB is None:
        _LIB = _try_load()
    return _LIB is not None


def stream_ptr() -> int:
    import torch
    return torch.cuda.current_stream().cuda_stream
