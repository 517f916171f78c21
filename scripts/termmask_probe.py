#!/usr/bin/env python3
"""term_bitmask microbenchmark (csrc/termmask.hip) at the bench shape,
1.25M documents and B = 128 term rows, on the synthetic Zipf corpus:

  (a) one exclude operand per row, a term with df ~ 10 % of the corpus
  (b) 16 operands per row: 8 require (the 8 terms with df nearest 50 %)
      and 8 exclude (df nearest 1 %)

The kernel alone: the entry point through ctypes on preallocated buffers,
device events around back-to-back launches (the fill of `out` from the
base rows is not in the window), median [min, max] over the rounds. Then
the masked BM25 step (search_bm25 with a live-only mask forced by one
tombstone) without operators and with the operands of (a) and (b), host
clock around synchronised batches.

Usage (GPU box): python scripts/termmask_probe.py [--docs N] [--batch B]
"""
from __future__ import annotations

import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_250_000)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--k", type=int, default=100)
    args = ap.parse_args()

    from infomesh_amd.ops import _build
    _build.build()
    from infomesh_amd.index.doc_attrs import TermOps
    from infomesh_amd.index.gpu_index import GpuShard
    from infomesh_amd.index.synth import synth_corpus_arrays, synth_queries
    from infomesh_amd.ops import _ext
    from infomesh_amd.ops import kernels as K

    dev = "cuda"
    N, B = args.docs, args.batch
    t0 = time.perf_counter()
    terms, docs, lens = synth_corpus_arrays(N, 120, seed=0)
    shard = GpuShard(dev)
    shard.build_from_arrays(terms, docs, lens, np.arange(N, dtype=np.int64),
                            None)
    torch.cuda.synchronize()
    seg = shard.segments[0]
    print(f"build: {time.perf_counter() - t0:.1f}s  N={N}  "
          f"postings={seg.doc_ids.numel()}  block={K.term_block_docs()}",
          flush=True)

    def nearest(share: float, n: int) -> list[int]:
        order = np.argsort(np.abs(shard.df - share * N), kind="stable")
        return [int(t) for t in order[:n]]

    cases = {
        "a: 1 exclude, df~10%": ([], nearest(0.10, 1)),
        "b: 8 require df~50% + 8 exclude df~1%": (nearest(0.50, 8),
                                                  nearest(0.01, 8)),
    }
    shard.delete([0])            # one tombstone: every batch is masked
    base = K.filter_bitmask(
        shard.attrs, torch.tensor([[0, -1, 0, 0]], dtype=torch.int32,
                                  device=dev))
    W = base.shape[1]
    src = torch.zeros(B, dtype=torch.int64, device=dev)
    lib = _ext.lib()
    for name, (req, exc) in cases.items():
        ids = np.asarray((req + exc) * B, dtype=np.int64)
        n_op = len(req) + len(exc)
        op_off = torch.arange(0, (B + 1) * n_op, n_op, dtype=torch.int32,
                              device=dev)
        kind = torch.tensor(([0] * len(req) + [1] * len(exc)) * B,
                            dtype=torch.int32, device=dev)
        begin = torch.from_numpy(seg.h_offs[ids]).to(dev)
        end = torch.from_numpy(seg.h_offs[ids + 1]).to(dev)
        npost = int((seg.h_offs[ids + 1] - seg.h_offs[ids]).sum())
        out = base.index_select(0, src)

        def launch():
            lib.infomesh_term_bitmask(
                seg.doc_ids.data_ptr(), seg.doc_ids.numel(),
                op_off.data_ptr(), begin.data_ptr(), end.data_ptr(),
                kind.data_ptr(), B * n_op, out.data_ptr(), B, W, N, 0, N,
                _ext.stream_ptr())
        for _ in range(30):
            launch()
        torch.cuda.synchronize()
        us = []
        for _ in range(args.rounds):
            ev0, ev1 = torch.cuda.Event(True), torch.cuda.Event(True)
            ev0.record()
            for _ in range(args.launches):
                launch()
            ev1.record()
            torch.cuda.synchronize()
            us.append(ev0.elapsed_time(ev1) / args.launches * 1e3)
        print(f"term_bitmask {name}: {statistics.median(us):.1f} "
              f"[{min(us):.1f}, {max(us):.1f}] us  "
              f"df={[int(shard.df[t]) for t in (req + exc)[:3]]}...  "
              f"postings/launch={npost}  "
              f"({npost / statistics.median(us) / 1e3:.1f} G postings/s)  "
              f"row 0 keeps {int((out[0] != 0).sum())} non-zero words "
              f"of {W}", flush=True)

    qterms, _ = synth_queries(B, n_terms=4, seed=1, device=dev)
    scores = torch.empty(B, N, device=dev, dtype=torch.float32)
    steps = {"no operators": None}
    for name, (req, exc) in cases.items():
        steps[name] = [TermOps.of(req, exc)] * B
    for name, ops in steps.items():
        for _ in range(5):
            shard.search_bm25(qterms, args.k, scores_buf=scores, term_ops=ops)
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            for _ in range(20):
                shard.search_bm25(qterms, args.k, scores_buf=scores,
                                  term_ops=ops)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) / 20 * 1e3)
        print(f"masked search_bm25, {name}: {statistics.median(ms):.3f} "
              f"[{min(ms):.3f}, {max(ms):.3f}] ms/batch", flush=True)


if __name__ == "__main__":
    main()
