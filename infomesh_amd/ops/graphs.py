"""hipGraph capture for launch-bound inner loops (guide: capture
launch-bound inner loops in hipGraphs).

GraphedCallable wraps a tensor-in/tensor-out function of FIXED shapes:
first call(s) run eagerly for warmup, then the op sequence is captured
once via torch.cuda.CUDAGraph (hipGraph on ROCm) and replayed with
static input buffers. Our ctypes kernel launches record into the graph
because they launch on torch's current (capture) stream.
"""
from __future__ import annotations

import gc
import logging
from typing import Callable

import torch

log = logging.getLogger("infomesh.graphs")


class GraphedCallable:
    """Shape-keyed graph cache around fn(*tensors) -> tensor|tuple."""

    def __init__(self, fn: Callable, warmup: int = 3, enabled: bool = True):
        self.fn = fn
        self.warmup = warmup
        self.enabled = enabled and torch.cuda.is_available()
        self._cache: dict[tuple, tuple] = {}
        self._failed = False

    def _key(self, args: tuple[torch.Tensor, ...]) -> tuple:
        return tuple((tuple(a.shape), a.dtype) for a in args)

    def __call__(self, *args: torch.Tensor):
        if not self.enabled or self._failed:
            return self.fn(*args)
        key = self._key(args)
        entry = self._cache.get(key)
        if entry is None:
            try:
                entry = self._capture(args)
            except Exception as e:  # fall back to eager, once
                log.warning("graph capture failed (%s); running eager", e)
                self._failed = True
                return self.fn(*args)
            self._cache[key] = entry
        graph, static_in, static_out = entry
        for s, a in zip(static_in, args):
            s.copy_(a, non_blocking=True)
        graph.replay()
        return static_out

    def _capture(self, args: tuple[torch.Tensor, ...]):
        static_in = tuple(a.clone() for a in args)
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            for _ in range(self.warmup):
                out = self.fn(*static_in)
        torch.cuda.current_stream().wait_stream(stream)
        graph = torch.cuda.CUDAGraph()
        # No cyclic GC while the stream captures: a collection that
        # finalizes some earlier graph, stream or event calls into HIP
        # mid-capture, which aborts the process.
        gc_was_enabled = gc.isenabled()
        gc.disable()
        try:
            with torch.cuda.graph(graph):
                static_out = self.fn(*static_in)
        finally:
            if gc_was_enabled:
                gc.enable()
        del out
        return graph, static_in, static_out
