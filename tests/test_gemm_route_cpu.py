"""gemm_nt's choice among the gemv, gemm8 and gemm kernel families is a
pure function of the shape; pin its boundaries (no GPU needed)."""
from __future__ import annotations

import pytest

from infomesh_amd.ops.kernels import gemm_route


def test_gemv_boundary():
    assert gemm_route(16, 4096, 3072, 1) == "gemv"
    assert gemm_route(17, 4096, 3072, 1) == "gemm"
    # M decides alone: a shape that would otherwise fill gemm8
    assert gemm_route(16, 1 << 20, 64, 64) == "gemv"


def test_gemm8_tile_count_boundary():
    """gemm8 needs ceil(M/256) * ceil(N/256) * G >= 224. With its other
    conditions (M >= 4096, N >= 512: at least 16 x 2 tiles) a count of
    223, a prime, cannot occur, so the count is isolated at 222 and the
    223-tile shape below also has N < 512."""
    assert gemm_route(4096, 3584, 128, 1) == "gemm8"       # 16*14 = 224
    assert gemm_route(4096, 512, 128, 7) == "gemm8"        # 16*2*7 = 224
    assert gemm_route(37 * 256, 1536, 128, 1) == "gemm"    # 37*6 = 222
    assert gemm_route(37 * 256, 512, 128, 3) == "gemm"     # 37*2*3 = 222
    assert gemm_route(223 * 256, 256, 128, 1) == "gemm"    # 223*1 = 223
    assert gemm_route(4096, 3584 - 256, 128, 1) == "gemm"  # 16*13 = 208
    # partial tiles count as whole ones
    assert gemm_route(4097, 3330, 192, 1) == "gemm8"       # 17*14 = 238
    # the other conditions at a sufficient tile count
    assert gemm_route(4095, 1 << 16, 128, 1) == "gemm"
    assert gemm_route(1 << 16, 511, 128, 8) == "gemm"


def test_gemm8_needs_whole_64_deep_k_steps():
    assert gemm_route(4096, 3584, 128 + 32, 1) == "gemm"
    assert gemm_route(4096, 3584, 128 + 64, 1) == "gemm8"


@pytest.mark.parametrize("M,N,K", [(4096, 1152, 384), (4096, 384, 384),
                                   (4096, 1536, 384), (4096, 384, 1536)])
def test_encoder_shapes_stay_on_gemm(M, N, K):
    """qkv / attn-out / ffn1 / ffn2 at B=128, S=32
    (scripts/gemm_tile_probe.py)."""
    assert gemm_route(M, N, K, 1) == "gemm"


def test_reranker_shape_runs_gemm8():
    assert gemm_route(512000, 2304, 768, 1) == "gemm8"
