"""Shapes, scores and masks shared by the GPU tests of the kernels over a
query row's whole match set (test_facets_gpu.py, test_top_domains_gpu.py,
test_collapse_gpu.py)."""
from __future__ import annotations

import numpy as np
import torch

B = 4
GARBAGE = 3.0e38        # the skipped row: every document would match
SCORES = np.asarray([0.0, -0.0, -1.0, 1.5e-30, 0.75, 2.0e30],
                    dtype=np.float32)


def _u(values) -> torch.Tensor:
    return torch.from_numpy(np.asarray(values, dtype=np.uint32)
                            .reshape(-1).view(np.int32))


def _size(name: str, CH: int) -> int:
    """N by name; CH is the kernels' chunk (documents per workgroup)."""
    return {"1": 1, "63": 63, "64": 64, "65": 65, "255": 255, "256": 256,
            "257": 257, "C-1": CH - 1, "C": CH, "C+1": CH + 1,
            "2C+37": 2 * CH + 37}[name]


def _mask(N: int, CH: int, rng) -> torch.Tensor:
    """Three mask rows: random bits with zero words at every chunk's
    first and last 128-byte score line; all zero; all ones."""
    W = (N + 63) // 64 * 2
    ok = np.zeros((3, W * 32), dtype=bool)
    ok[0, :N] = rng.random(N) < 0.6
    ok[2, :N] = True
    words = np.packbits(ok, axis=1, bitorder="little").view(np.uint32) \
        .reshape(3, W).copy()
    if N > 64:                # (at N <= 64 that would leave nothing)
        for c0 in range(0, N, CH):
            words[0, c0 // 32] = 0
            words[0, (min(c0 + CH, N) - 1) // 32] = 0
    return torch.from_numpy(words.view(np.int32))
