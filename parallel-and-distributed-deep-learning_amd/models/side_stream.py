"""The two-stream backward's scheduler, shared by the bf16 and fp32 HIP engines.

Weight gradients run on a side stream concurrently with the data-gradient chain on the compute
stream; this mixin orders the two.  Its state lives on the engine itself (`side`, `_evpool`,
`_evi`, `_pending`, `_last_side`, `_defer`): train/graph.py and the strategies read and assign
`side` and `_defer` there.  What differs between the engines stays with them: whether a side
stream is wanted (`_two_stream_wanted`), the ring depths, `defer_side`, and how a finished
bucket is reported (`_bucket_ready` here, or `_join_side` and a call on the compute stream).

tests/test_side_stream_cpu.py drives this protocol with fake streams and events.
"""
from __future__ import annotations

import torch


class SideStream:
    def _init_side(self, dev, two_stream):
        self.side = torch.cuda.Stream(dev) if two_stream and dev.type == "cuda" else None
        self._evpool, self._evi = [], 0   # fork/join events (see _event)
        self._pending, self._last_side = {}, None
        self._defer = None            # capture-time list of deferred side-stream closures

    def _side_begin_step(self):
        """A new step: no side-stream reader is outstanding, and the event pool starts over."""
        self._pending, self._last_side = {}, None
        self._evi = 0

    def _event(self):
        """The next fork/join event of this step, from a pool the engine owns for its whole
        life: the i-th record of every step reuses the i-th event (a wait binds to the record
        made before it, so reuse after the wait is safe), so a step -- eager or captured --
        creates and destroys no HIP events."""
        i = self._evi
        self._evi += 1
        if i == len(self._evpool):
            self._evpool.append(torch.cuda.Event())
        return self._evpool[i]

    def _side_run(self, fn, *args, reads=()):
        """Launch a weight-gradient kernel on the side stream, ordered after everything enqueued
        on the compute stream so far; `reads` names the gradient buffers it reads, which the
        compute stream must not overwrite before it is done (see _before_write).

        Deferred (a segmented capture, begin_defer): the call is queued instead, and the capture
        records the queue of each segment as a single-stream side graph that the replay runs
        after that segment's main graph, concurrently with the next segment.  No fork / join
        events inside any graph (the runtime launches single-stream graphs from pre-built packets;
        its multi-branch launch path faults: train/graph.py replay_stream), and no buffer hazards:
        the deferred engine's gradient buffers are never reused within a step (_alloc_acts)."""
        if self._defer is not None:
            self._defer.append((fn, args))
            return
        if self.side is None:
            fn(*args)
            return
        main = torch.cuda.current_stream(self.device)
        ev = self._event()
        ev.record(main)
        self.side.wait_event(ev)
        with torch.cuda.stream(self.side):
            fn(*args)
        done = self._event()
        done.record(self.side)
        for r in reads:
            self._pending[r] = done
        self._last_side = done

    def _before_write(self, *bufs):
        """The compute stream is about to overwrite these gradient buffers: wait for the side
        stream's last reader of each."""
        if self.side is None or self._defer is not None:
            return
        main = torch.cuda.current_stream(self.device)
        for b in bufs:
            ev = self._pending.pop(b, None)
            if ev is not None:
                main.wait_event(ev)

    def _bucket_ready(self, cb, i):
        """Report bucket i complete.  Two streams: its gradients come from both streams, so the
        side stream first waits for the compute stream and the callback runs with the SIDE stream
        current -- whatever it enqueues or records (an all-reduce, an optimizer update) is
        ordered after both, and the compute stream never blocks on the side stream."""
        if self.side is None or self._defer is not None:
            cb(i)
            return
        if getattr(cb, "needs_join", False):   # (e.g. a graph capture cut at the bucket boundary)
            self._join_side()
            cb(i)
            return
        ev = self._event()
        ev.record(torch.cuda.current_stream(self.device))
        self.side.wait_event(ev)
        with torch.cuda.stream(self.side):
            cb(i)
        done = self._event()
        done.record(self.side)
        self._last_side = done

    def begin_defer(self):
        """Queue side-stream work from now on (segmented capture; take_deferred drains it)."""
        assert self.side is not None and self.defer_side
        self._defer = []

    def take_deferred(self):
        q, self._defer = self._defer, []
        return q

    def end_defer(self):
        left, self._defer = self._defer, None
        assert not left, "deferred side work left uncaptured"

    def _join_side(self):
        if self.side is None or self._last_side is None:
            return
        torch.cuda.current_stream(self.device).wait_event(self._last_side)
        self._pending.clear()
        self._last_side = None
