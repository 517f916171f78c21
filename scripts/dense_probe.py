#!/usr/bin/env python3
"""Dense-plane probe: time the scoring GEMM + top-k at flagship shapes.
Round-1 baseline: 529 us at 128x1.25Mx384 (~3.1 TB/s effective) vs a
~5.4 TB/s measured mixed ceiling (BACKLOG / VERDICT #6).
--pruned times the pair the dense plane runs today instead: the GEMM
that also writes block maxima and the selector that reads them.
--compare-lib OTHER.so times the pruned selector alone, this build and
another build of the extension alternately in one process (device
events, 7 rounds of 10 calls each, median [min, max] per call), and
compares their outputs."""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def _stats(us: list[float]) -> str:
    us = sorted(us)
    return f"{us[len(us) // 2]:.1f} [{us[0]:.1f}, {us[-1]:.1f}] us"


def compare_selector(args) -> None:
    """The selector on GEMM scores and maxima, this build against
    args.compare_lib. A build that still exports a workspace length for
    the pruned selector gets that workspace and its zero fill inside the
    timed call, as its wrapper did. Each timed group of calls is queued
    behind two GEMMs, so the events bracket device time and not the
    host's launch rate."""
    from ctypes import c_int, c_long
    from infomesh_amd.ops import _ext
    from infomesh_amd.ops import kernels as K
    dev = "cuda"
    M, N, D, k = args.batch, args.docs, args.dim, args.k
    a = torch.randn(M, D, device=dev).bfloat16()
    b = torch.randn(N, D, device=dev).bfloat16()
    scores, bmax, W = K.gemm_nt_bmax(a, b)
    other = _ext.bind(args.compare_lib, strict=False)
    ws, nzero = None, 0
    if hasattr(other, "infomesh_topk_pruned_workspace_u32"):
        other.infomesh_topk_pruned_workspace_u32.restype = c_long
        other.infomesh_topk_pruned_workspace_u32.argtypes = [c_int, c_long,
                                                             c_int, c_int]
        other.infomesh_topk_pruned_zero_u32.restype = c_long
        other.infomesh_topk_pruned_zero_u32.argtypes = [c_int]
        ws = torch.empty(other.infomesh_topk_pruned_workspace_u32(M, N, k, W),
                         device=dev, dtype=torch.int32)
        nzero = other.infomesh_topk_pruned_zero_u32(M)
    tkp = K.TopKPruned(dev)

    def this():
        return tkp(scores, bmax, W, k)

    def that():
        if nzero:
            ws[:nzero].zero_()
        vals = torch.empty((M, k), device=dev, dtype=torch.float32)
        idx = torch.empty((M, k), device=dev, dtype=torch.int32)
        other.infomesh_topk_pruned(
            scores.data_ptr(), bmax.data_ptr(), W,
            0 if ws is None else ws.data_ptr(), vals.data_ptr(),
            idx.data_ptr(), M, N, k, _ext.stream_ptr())
        return vals, idx

    (v0, i0), (v1, i1) = this(), that()
    torch.cuda.synchronize()
    print(f"selector {M} x {N}, k={k}, W={W}: values equal "
          f"{torch.equal(v0, v1)}, indices equal {torch.equal(i0, i1)} "
          f"({int((i0 != i1).sum())} differ)")
    times = {"this build": [], "other build": []}
    for _ in range(7):
        for name, fn in (("this build", this), ("other build", that)):
            fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
            for _ in range(2):
                K.gemm_nt_bmax(a, b, out=scores, bmax=bmax)
            e0.record()
            for _ in range(10):
                fn()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) * 100.0)   # us per call
    for name, us in times.items():
        print(f"topk pruned, {name}: {_stats(us)}")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_250_000)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--pruned", action="store_true",
                    help="GEMM with block maxima + pruned top-k")
    ap.add_argument("--compare-lib", metavar="OTHER.so",
                    help="time the pruned selector against another build")
    args = ap.parse_args()
    from infomesh_amd.ops import _build
    _build.build()
    from infomesh_amd.ops import kernels as K
    if args.compare_lib:
        compare_selector(args)
        return

    dev = "cuda"
    M, N, D = args.batch, args.docs, args.dim
    a = torch.randn(M, D, device=dev).bfloat16()
    b = torch.randn(N, D, device=dev).bfloat16()
    out = torch.empty(1, M, N, device=dev, dtype=torch.float32)
    tk = K.TopK(dev)

    # parity spot-check first
    got = K.gemm_nt(a, b, out_f32=True, out=out).reshape(M, N)
    ref = (a[:4].float() @ b[:4096].float().T)
    err = (got[:4, :4096] - ref).abs().max().item()
    print(f"parity max err (4x4096 slice): {err:.4f}")

    gemm_gb = (N * D * 2 + M * D * 2 + M * N * 4) / 1e9
    if args.pruned:
        W = K.gemm_bmax_width(M, N, D)
        assert W, "shape has no block-maxima GEMM"
        NB = (N + W - 1) // W
        bmax = torch.empty(M, NB, device=dev, dtype=torch.float32)
        tkp = K.TopKPruned(dev)
        out2d = out.reshape(M, N)
        K.gemm_nt_bmax(a, b, out=out2d, bmax=bmax)
        assert torch.equal(bmax[:, :-1],
                           out2d[:, :(NB - 1) * W].view(M, NB - 1, W)
                           .amax(dim=2)), "block maxima differ"
        # bytes moved: the GEMM writes the maxima once; the selector
        # streams them three times (hist1, hist2, compact), reads
        # min(k, NB) blocks of W scores and writes them side by side,
        # and streams that copy three times — no term in M * N
        bmax_gb = M * NB * 4 / 1e9
        sel_gb = 3 * bmax_gb + 5 * M * min(args.k, NB) * W * 4 / 1e9
        cases = [
            ("gemm+bmax", gemm_gb + bmax_gb,
             lambda: K.gemm_nt_bmax(a, b, out=out2d, bmax=bmax)),
            ("topk pruned", sel_gb, lambda: tkp(out2d, bmax, W, args.k)),
            ("gemm+bmax+topk pruned", gemm_gb + bmax_gb + sel_gb,
             lambda: tkp(*K.gemm_nt_bmax(a, b, out=out2d, bmax=bmax),
                         args.k)),
        ]
    else:
        cases = [
            ("gemm", gemm_gb, lambda: K.gemm_nt(a, b, out_f32=True, out=out)),
            ("topk", 3 * M * N * 4 / 1e9,
             lambda: tk(out.reshape(M, N), args.k)),
            ("gemm+topk", (N * D * 2 + 4 * M * N * 4) / 1e9,
             lambda: tk(K.gemm_nt(a, b, out_f32=True,
                                  out=out).reshape(M, N), args.k)),
        ]
    for name, gb, fn in cases:
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / args.iters
        print(f"{name}: {ms * 1e3:.0f} us  ({gb / (ms / 1e3):.2f} GB/s)")


if __name__ == "__main__":
    main()
