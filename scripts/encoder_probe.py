#!/usr/bin/env python3
"""Encoder forward probe: bge-small-shaped batch encode latency.
Round-1 baseline ~1.2 ms/batch at B=128,S=32 (VERDICT #6 target <0.8).

--compare times the plain kernel sequence (fast_path=False) against the
fast path, and the fast path with each single item taken out, in one
process: the configurations alternate within every round, device events
around --iters graph replays, and the table gives the median [min, max]
of the rounds' per-batch times."""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def _inputs(batch: int, seq: int):
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(4, 30522, (batch, seq), generator=g,
                        dtype=torch.int32).cuda()
    ids[:, 0] = 1
    lens = torch.full((batch,), seq, dtype=torch.int32, device="cuda")
    return ids, lens


def compare(args) -> None:
    import statistics

    from infomesh_amd.models.bert import FAST_ITEMS
    from infomesh_amd.models.encoder import EmbeddingEncoder

    ids, lens = _inputs(args.batch, args.seq)
    configs = {"plain": frozenset(), "fast": FAST_ITEMS}
    for item in sorted(FAST_ITEMS):
        configs[f"fast-{item}"] = FAST_ITEMS - {item}
    encs = {name: EmbeddingEncoder(device="cuda", fast_path=items)
            for name, items in configs.items()}
    ref = encs["plain"].encode_ids(ids, lens).clone()
    for name, enc in encs.items():
        same = torch.equal(enc.encode_ids(ids, lens), ref)
        print(f"{name}: output {'identical to' if same else 'DIFFERS from'}"
              " plain")
        for _ in range(10):
            enc.encode_ids(ids, lens)
    torch.cuda.synchronize()
    times: dict[str, list[float]] = {name: [] for name in encs}
    for _ in range(args.rounds):
        for name, enc in encs.items():
            e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
            e0.record()
            for _ in range(args.iters):
                enc.encode_ids(ids, lens)
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / args.iters * 1e3)
    print(f"encode B={args.batch} S={args.seq}, {args.rounds} rounds x "
          f"{args.iters} iters, us/batch: median [min, max]")
    for name, t in times.items():
        print(f"  {name:12s} {statistics.median(t):7.1f} "
              f"[{min(t):7.1f}, {max(t):7.1f}]")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--seq", type=int, default=32)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--compare", action="store_true",
                    help="plain path vs fast path vs fast path minus "
                         "each item, alternating")
    ap.add_argument("--rounds", type=int, default=9)
    args = ap.parse_args()
    from infomesh_amd.ops import _build
    _build.build()
    from infomesh_amd.models.encoder import EmbeddingEncoder
    if args.compare:
        compare(args)
        return

    enc = EmbeddingEncoder(device="cuda")
    ids, lens = _inputs(args.batch, args.seq)
    # parity vs CPU fp32 reference on a small slice
    out = enc.encode_ids(ids, lens)
    ref = enc.encode_ids_reference(ids[:4].cpu(), lens[:4].cpu())
    err = (out[:4].cpu().float() - ref.float()).abs().max().item()
    print(f"parity vs fp32 reference (4 rows): max err {err:.4f}")
    for _ in range(10):
        enc.encode_ids(ids, lens)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    e0.record()
    for _ in range(args.iters):
        enc.encode_ids(ids, lens)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / args.iters
    print(f"encode B={args.batch} S={args.seq}: {ms * 1e3:.0f} us/batch")


if __name__ == "__main__":
    main()
