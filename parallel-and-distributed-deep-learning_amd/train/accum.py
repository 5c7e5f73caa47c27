"""Gradient accumulation: one update from k micro-batches (--accum-steps, Horovod's
`backward_passes_per_step` of DistributedOptimizer, imagenet-resnet50-hvd.py:101 [lib]).

Every `train_step` is a micro-step that scales its loss by 1 / (B * replicas * k), so the sum of
the k micro-batch gradients IS the mean gradient over the k * B * replicas images and nothing is
rescaled afterwards.  The running sum lives in `acc`, a second buffer shaped like
`engine.grads` (+102 MB per replica for ResNet-50), maintained by one streaming kernel
(`grad_accum`, csrc/kernels/optim.hip) in three modes:

    micro-step 1        store  acc  = g       (no memset; a bitwise copy)
    micro-steps 2..k-1  add    acc += g
    micro-step k        fold   g   += acc     (in place: the all-reduce and the optimizers keep
                                               reading `engine.grads`)

so the order of additions is fixed, ((g1 + g2) + ...) + gk, and replicas that see identical
data stay bit-identical.  With a communication callback the three run per bucket inside the
engine's `bucket_cb`, i.e. on the stream the engine makes current for it (the side stream of a
two-stream step) and, on micro-step k, before the bucket is handed to the all-reduce.  Only
micro-step k communicates.  Without one (no collective to run) a single whole-buffer call
after `forward_backward` does the same.  On CPU tensors the three operations are torch ops.

Train-mode BN normalises every micro-batch with its own statistics and advances the moving
statistics on every micro-step (the usual semantics of accumulation: k micro-batches of B are
not one batch of k * B for BN).
"""
from __future__ import annotations

from typing import Callable, List, Optional, Tuple

import torch

STORE, ADD, FOLD = 0, 1, 2


def check_accum_steps(k) -> int:
    if int(k) != k or int(k) < 1:
        raise ValueError(f"--accum-steps must be an integer >= 1 (got {k!r})")
    return int(k)


class GradAccumulator:
    def __init__(self, engine, k: int, buckets: Optional[List[Tuple[int, int]]] = None):
        self.k = check_accum_steps(k)
        if self.k < 2:
            raise ValueError("GradAccumulator is for k >= 2 (k = 1 allocates and launches nothing)")
        self.engine = engine
        self.grads = engine.grads
        self.acc = torch.empty_like(engine.grads)
        self.buckets = list(buckets) if buckets is not None else None
        self.micro = 0               # micro-steps completed since the last update
        self._ev = torch.cuda.Event() if self.grads.is_cuda else None
        self._pending = False        # callbacks of this micro-step ran (on whatever stream was current)

    @property
    def last(self) -> bool:
        """Whether the micro-step now running (or about to run) is the k-th: the one that
        communicates and updates."""
        return self.micro == self.k - 1

    def _mode(self) -> int:
        return STORE if self.micro == 0 else (FOLD if self.last else ADD)

    def _apply(self, mode: int, s: int, e: int):
        acc, g = self.acc[s:e], self.grads[s:e]
        if g.is_cuda:
            from ..ops.native import native
            native.grad_accum(acc, g, mode)      # (current stream)
        elif mode == STORE:
            acc.copy_(g)
        elif mode == ADD:
            acc.add_(g)
        else:
            g.add_(acc)

    def wrap(self, comm_cb: Callable[[int], None]) -> Callable[[int], None]:
        """The engine's bucket callback for this micro-step: accumulate bucket i; on the k-th
        micro-step fold it and only then report it to `comm_cb`."""
        if self.buckets is None:
            raise ValueError("GradAccumulator.wrap needs the bucket layout")
        mode, last = self._mode(), self.last

        def cb(i):
            s, e = self.buckets[i]
            self._apply(mode, s, e)
            if self._ev is not None:
                self._ev.record(torch.cuda.current_stream(self.grads.device))
                self._pending = True
            if last:
                comm_cb(i)
        return cb

    def accumulate(self):
        """Whole buffer in one call (no communication callback), after `forward_backward`."""
        self._apply(self._mode(), 0, self.grads.numel())

    def advance(self) -> bool:
        """End of a micro-step, called after `forward_backward` on the stream that ran it; True
        when it was the k-th (the update is due).  The engine does not join the stream its
        callbacks ran on, so the caller's stream waits here for the last bucket's accumulation:
        the next micro-step may overwrite `grads` from either stream."""
        if self._pending:
            torch.cuda.current_stream(self.grads.device).wait_event(self._ev)
            self._pending = False
        self.micro += 1
        if self.micro == self.k:
            self.micro = 0
            return True
        return False
