"""Route half of the CLS-only tail's same-kernel rule (no GPU needed):
the tail's three GEMMs at M = B and the full layer's at M = B*S must
both run the gemm.hip family; the tile half needs the extension and is
checked in test_encoder_fastpath_gpu.py."""
from __future__ import annotations

import pytest

from infomesh_amd.models.bert import cls_tail_gemms, cls_tail_routes_match
from infomesh_amd.models.encoder import BGE_SMALL
from infomesh_amd.ops.kernels import gemm_route

H, F = BGE_SMALL.hidden, BGE_SMALL.ffn


def test_tail_gemm_shapes():
    assert cls_tail_gemms(H, F) == ((384, 384), (1536, 384), (384, 1536))


@pytest.mark.parametrize("B,rows,same", [
    (128, 4096, True),     # the benchmark batch
    (16, 512, False),      # 8-GPU sharded encode: the tail would be gemv
    (64, 2048, True),      # same family; the tile half tells them apart
])
def test_route_half(B, rows, same):
    assert cls_tail_routes_match(B, rows, H, F) is same
    for N, K in cls_tail_gemms(H, F):
        assert gemm_route(rows, N, K, 1) == "gemm"
        assert gemm_route(B, N, K, 1) == ("gemv" if B <= 16 else "gemm")


def test_route_half_refuses_gemm8_rows():
    """A full layer on the 256x256 tile kernel has no tail twin."""
    assert gemm_route(1 << 16, F, H, 1) == "gemm8"
    assert not cls_tail_routes_match(2048, 1 << 16, H, F)
